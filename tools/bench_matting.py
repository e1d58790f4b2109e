#!/usr/bin/env python3
"""The blur-fusion foreground estimator and the BiRefNet cutout on one MI355X; prints one JSON line:
per-launch device times (HIP events, median) of the estimator's four launches -- horizontal and vertical, radius 30 then radius 3 -- for rgb_u8 images and
an rgba_u8 result at 1024^2 and 2048^2, batch 8; for each launch the bytes it must move (every operand once) over the float4-copy rate of the
part (6.29 TB/s, MI355X_MICROARCH.md) as `bound_ms`, and measured / bound as `x_bound`; then the cutout step against the BiRefNet step alone on the same
BiRefNet-lite model (synthetic weights) at 1024^2, batch 8. Nothing is asserted: one run on one machine.
Usage: python tools/bench_matting.py [--iters 20] [--no-model]"""
import argparse
import json
import sys
import tempfile
import time
from ctypes import byref, c_float, c_void_p
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from __graft_entry__ import load_package  # noqa: E402

load_package()
import dataclasses  # noqa: E402

from visioncpp_amd import _lib as L  # noqa: E402
from visioncpp_amd import synth, vision  # noqa: E402
from visioncpp_amd.vision import DeviceBuffer  # noqa: E402
from visioncpp_amd.vision import ImageFormat as F  # noqa: E402

COPY = 6.29e12  # bytes/s, measured float4 copy
# bytes per pixel each launch must move: reads + writes, every operand once
BYTES = {"r30_h": 3 + 4 + 32, "r30_v": 32 + 3 + 4 + 16 + 16, "r3_h": 16 + 16 + 4 + 32, "r3_v": 32 + 3 + 4 + 4}


def event_ms(api, fn, iters):
    a, b, ms = c_void_p(), c_void_p(), c_float()
    L.vx_check(api.vx_event_create(byref(a)))
    L.vx_check(api.vx_event_create(byref(b)))
    ts = []
    for _ in range(iters):
        L.vx_check(api.vx_event_record(a, None))
        fn()
        L.vx_check(api.vx_event_record(b, None))
        L.vx_check(api.vx_event_elapsed_ms(a, b, byref(ms)))
        ts.append(ms.value)
    api.vx_event_destroy(a)
    api.vx_event_destroy(b)
    return float(np.median(ts))


def wall_ms(fn, iters):
    ts = []
    for _ in range(iters):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def launches(api, size, batch, iters):
    rng = np.random.default_rng(size)
    n = batch * size * size
    img = DeviceBuffer.from_numpy(rng.integers(0, 256, (n, 3), dtype=np.uint8))
    mask = DeviceBuffer.from_numpy(rng.random(n, dtype=np.float32))
    planes, fg1, bg1, out = DeviceBuffer(n * 32), DeviceBuffer(n * 16), DeviceBuffer(n * 16), DeviceBuffer(n * 4)
    u8, f32 = F.rgba_u8.value, F.rgba_f32.value

    def stage(radius, second, passes):
        return lambda: L.vx_check(api.vx_foreground_stage(img.ptr, F.rgb_u8.value, fg1.ptr if second else None, bg1.ptr if second else None, mask.ptr, planes.ptr,
                                                          out.ptr if second else fg1.ptr, u8 if second else f32, None if second else bg1.ptr, batch, size, size,
                                                          radius, passes, None))

    rows = {}
    for name, fn in (("r30_h", stage(30, False, 1)), ("r30_v", stage(30, False, 2)), ("r3_h", stage(3, True, 1)), ("r3_v", stage(3, True, 2))):
        fn()
        ms = event_ms(api, fn, iters)
        bound = n * BYTES[name] / COPY * 1e3
        rows[name] = dict(ms=round(ms, 4), bound_ms=round(bound, 4), x_bound=round(ms / bound, 2))
    rows["all_four_ms"] = round(sum(r["ms"] for r in rows.values()), 4)
    rows["ms_per_image"] = round(rows["all_four_ms"] / batch, 4)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--no-model", action="store_true", help="skip the BiRefNet-lite comparison")
    a = ap.parse_args()
    dev = vision.Device.init(vision.Backend.gpu)
    api = L.get_lib()
    out = dict(what="blur-fusion foreground estimator, rgb_u8 -> rgba_u8, radius 30 then 3, batch 8", copy_rate_TBps=COPY / 1e12)
    for size in (1024, 2048):
        out[f"launches_{size}"] = launches(api, size, 8, a.iters)
    if not a.no_model:
        B, S = 8, 1024
        cfg = dataclasses.replace(synth.SWIN_T, image_size=S)
        with tempfile.TemporaryDirectory() as td:
            model = vision.Model.load(synth.write_birefnet_gguf(Path(td) / "lite.gguf", cfg, seed=4), dev, vision.Arch.birefnet)
        rgb = DeviceBuffer.from_numpy(synth.images(B, S, S, seed=64))
        mask, rgba = DeviceBuffer(B * S * S * 4), DeviceBuffer(B * S * S * 4)
        step = lambda: model.segment_batch_device(rgb.ptr, B, S, S, mask.ptr)  # noqa: E731
        cut = lambda: model.birefnet_cutout_batch_device(rgb.ptr, B, S, S, rgba.ptr, 30)  # noqa: E731
        for fn in (step, cut):
            fn()
            fn()
        t_step, t_cut = wall_ms(step, a.iters), wall_ms(cut, a.iters)
        out["birefnet_lite_1024_b8"] = dict(step_ms=round(t_step, 3), cutout_ms=round(t_cut, 3), cutout_over_step=round(t_cut / t_step, 3),
                                           images_per_s_step=round(B / t_step * 1e3, 1), images_per_s_cutout=round(B / t_cut * 1e3, 1))
    print(json.dumps(out))


if __name__ == "__main__":
    main()

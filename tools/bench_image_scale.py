#!/usr/bin/env python3
"""image_scale on one MI355X against the host function it restates, and Depth-Anything's any-extent entry against the depthany_compute loop;
prints one JSON line. Times are host clocks around calls that end in a device synchronise, medians over --iters.
  scale_in / scale_out: rgb_u8 w x h -> the model's extent for it, and alpha_f32 back. `device_ms_per_image`: visp_image_scale_batch_device on
    device-resident arrays at --batch, over the batch -- the whole entry: tap tables made and uploaded, one launch, synchronise.
    `host_ms_per_image`: visp_image_scale, one image (the baseline: what every caller pays today, before the two PCIe trips).
  depthany: visp_depthany_compute_scaled_batch_device at --batch on device-resident images against visp_model_compute (depthany_compute, then its u8 map) image by image on
    the same inputs (--baseline-images of them, it is the slow side), both per image. Synthetic weights of the Small configuration.
Nothing is asserted: one run on one machine. Usage: python tools/bench_image_scale.py [--w 1920 --h 1080 --batch 32 --iters 10] [--no-model]"""
import argparse
import json
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from __graft_entry__ import load_package  # noqa: E402

load_package()
from visioncpp_amd import synth, vision  # noqa: E402
from visioncpp_amd.vision import DeviceBuffer  # noqa: E402
from visioncpp_amd.vision import ImageFormat as F  # noqa: E402


def wall_ms(fn, iters):
    ts = []
    for _ in range(iters):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def scale_row(dev, src, fmt, ow, oh, iters):
    b, h, w = src.shape[:3]
    x, y = DeviceBuffer.from_numpy(src), DeviceBuffer(b * oh * ow * src[0, 0, 0].nbytes)
    on_device = lambda: vision.image_scale_batch_device(x.ptr, fmt, b, w, h, y.ptr, ow, oh, device=dev)  # noqa: E731
    on_host = lambda: vision.image_scale(src[0], ow, oh, fmt)  # noqa: E731
    on_device()
    d, hst = wall_ms(on_device, iters) / b, wall_ms(on_host, max(2, iters // 3))
    return dict(format=fmt.name, source=[w, h], target=[ow, oh], batch=b, device_ms_per_image=round(d, 4), host_ms_per_image=round(hst, 3), host_over_device=round(hst / d, 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--w", type=int, default=1920)
    ap.add_argument("--h", type=int, default=1080)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--baseline-images", type=int, default=4)
    ap.add_argument("--no-model", action="store_true", help="the two scale rows only (the model's extent is computed from the Small configuration)")
    a = ap.parse_args()
    dev = vision.Device.init(vision.Backend.gpu)
    cfg = synth.SMALL
    side = max(cfg.image_size, -(-min(a.w, a.h) // 14) * 14)  # depthany_image_extent
    mw, mh = (-(-(a.w * side // min(a.w, a.h)) // 14) * 14, -(-(a.h * side // min(a.w, a.h)) // 14) * 14)
    imgs = synth.images(a.batch, a.w, a.h, seed=7)
    maps = np.random.default_rng(7).random((a.batch, mh, mw, 1), dtype=np.float32)
    out = dict(what="image_scale on the device against the host function; Depth-Anything any-extent entry against the depthany_compute loop", model_extent=[mw, mh])
    out["scale_in"] = scale_row(dev, imgs, F.rgb_u8, mw, mh, a.iters)
    out["scale_out"] = scale_row(dev, maps, F.alpha_f32, a.w, a.h, a.iters)
    if not a.no_model:
        with tempfile.TemporaryDirectory() as td:
            model = vision.Model.load(synth.write_gguf(Path(td) / "small.gguf", cfg, seed=0), dev)
        assert model.image_extent(a.w, a.h) == (mw, mh)
        x, y = DeviceBuffer.from_numpy(imgs), DeviceBuffer(a.batch * a.h * a.w * 4)
        scaled = lambda: model.compute_scaled_batch_device(x.ptr, a.batch, a.w, a.h, y.ptr)  # noqa: E731
        n = min(a.baseline_images, a.batch)
        loop = lambda: [model.compute(imgs[i]) for i in range(n)]  # noqa: E731
        scaled()
        loop()
        t_scaled, t_loop = wall_ms(scaled, max(3, a.iters // 2)) / a.batch, wall_ms(loop, 3) / n
        out["depthany"] = dict(batch=a.batch, scaled_batch_device_ms_per_image=round(t_scaled, 3), compute_loop_ms_per_image=round(t_loop, 3), baseline_images=n,
                               loop_over_scaled=round(t_loop / t_scaled, 2))
    print(json.dumps(out))


if __name__ == "__main__":
    main()

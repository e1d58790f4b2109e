#!/usr/bin/env python3
"""MI-GAN 512-places2-shaped generator (synthetic weights, real channel table) on one MI355X; prints one JSON line:
batch-1 latency of migan_compute (host image + mask -> host rgba), batch-1 device time of the graph-replayed batch entry,
images/s at batch 8 and 16, FLOPs and bytes per image (summed from the schedule's own per-launch accounting) and the share
of the HBM byte bound (6.3 TB/s achievable, MI355X_MICROARCH.md) the batched run reaches.
Usage: python tools/bench_migan.py [--res 512] [--iters 20] [--timing]"""
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
from visioncpp_amd import _lib as L  # noqa: E402
from visioncpp_amd import synth  # noqa: E402
from visioncpp_amd.vision import Backend, Device, DeviceBuffer, Migan  # noqa: E402

HBM = 6.3e12


def inputs(n: int, res: int):
    imgs = synth.images(n, res, res, seed=3)
    masks = np.zeros((n, res, res), np.uint8)
    masks[:, res // 4:res // 2, res // 3:2 * res // 3] = 255
    return imgs, masks


def median_ms(fn, iters: int) -> float:
    ts = []
    for _ in range(iters):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--timing", action="store_true", help="also print the per-kernel-group table of one batch-16 call")
    a = ap.parse_args()
    dev = Device.init(Backend.gpu)
    with tempfile.TemporaryDirectory() as td:
        m = Migan.load(synth.write_migan_gguf(Path(td) / "m.gguf", a.res, seed=1), dev)
    res = a.res
    api = L.get_lib()
    img1, mask1 = inputs(1, res)
    m.compute(img1[0], mask1[0])
    lat = median_ms(lambda: m.compute(img1[0], mask1[0]), a.iters)
    out = dict(model=f"migan-{res} (synthetic weights)", channels=synth.migan_channels(res), compute_b1_ms=round(lat, 3))
    for b in (1, 8, 16):
        imgs, masks = inputs(b, res)
        din, dmask, dout = DeviceBuffer.from_numpy(imgs), DeviceBuffer.from_numpy(masks), DeviceBuffer(b * res * res * 4)
        run = lambda: L.check(api.visp_migan_compute_batch_device(m._handle, din.ptr, 3, dmask.ptr, b, dout.ptr, None))  # noqa: E731
        run()
        run()  # captured; replays from here on
        ms = median_ms(run, a.iters)
        if b == 1:
            out["device_b1_ms"] = round(ms, 3)
        else:
            out[f"images_per_s_b{b}"] = round(b / ms * 1e3, 1)
            out[f"ms_per_batch_b{b}"] = round(ms, 3)
        if b == 16:
            m.enable_timing(True)
            run()
            table = m.read_timing()
            m.enable_timing(False)
            flops = sum(t["flops"] for t in table) / b
            bytes_ = sum(t["bytes"] for t in table) / b
            out["gflop_per_image"] = round(flops / 1e9, 2)
            out["mb_per_image"] = round(bytes_ / 1e6, 1)
            out["byte_bound_ms_per_image"] = round(bytes_ / HBM * 1e3, 4)
            out["byte_bound_share_b16"] = round((bytes_ / HBM * 1e3) / (ms / b), 3)
            if a.timing:
                for t in table:
                    print(f"# {t['name']:12s} {t['ms']:8.3f} ms  launches {t['launches']:3d}  {t['bytes'] / max(t['ms'], 1e-9) / 1e6:8.1f} GB/s  "
                          f"{t['flops'] / max(t['ms'], 1e-9) / 1e6:8.1f} GFLOP/s")
    print(json.dumps(out))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Polygons to RLE on the device (kernels_rle_poly.hip) against rleFrPoly's loop on the host (csrc/mask_rle.cpp, visp_image_rle_from_poly_reference_host) on
the same input. Prints a text record and writes ONE JSON line to --out. A measurement, not a gate.

  1. --polygons synthetic COCO-like polygons at 640 x 480: 10 .. 200 vertices around a centre, radii of a few to a few hundred pixels with jitter.
  2. one long outline at 1024 x 1024: a --long-vertices zigzag from side to side (its keys pass the LDS sort: the global-memory sort path).
  Each: the three forms of vx_poly_rle by HIP events (stream NULL, buffers allocated once), vision.poly_to_rle (uploads, all passes, the rows as Python lists) and the host loop's C call by the
  host clock; the device rows are held equal to the host loop's before anything is timed.

    python tools/bench_mask_rle_poly.py [--warmup 2] [--samples 7] [--polygons 4000] [--long-vertices 400] [--out profiles/mask_rle_poly_bench.txt]"""
import argparse
import ctypes as C
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from __graft_entry__ import load_package  # noqa: E402

load_package()
from tests import gpu_util as U  # noqa: E402
from tools.bench_sam_regions import events_ms, stats  # noqa: E402
from visioncpp_amd import _lib as L  # noqa: E402
from visioncpp_amd import vision  # noqa: E402


def coco_like(count, w, h, seed=7):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(count):
        k = int(rng.integers(10, 201))
        centre, radius = rng.uniform((0, 0), (w, h)), float(np.exp(rng.uniform(np.log(4), np.log(250))))
        angle = np.sort(rng.uniform(0, 2 * np.pi, k))
        r = radius * rng.uniform(0.7, 1.3, k)
        out.append(np.round(np.stack([centre[0] + r * np.cos(angle), centre[1] + r * np.sin(angle)], 1), 2))
    return out


def host_loop(xy, poff, n, w, h):
    offsets, runs, owner = np.zeros(n + 1, np.int64), C.c_void_p(), C.c_void_p()
    L.check(L.get_lib().visp_image_rle_from_poly_reference_host(xy.ctypes.data, poff.ctypes.data, n, w, h, offsets.ctypes.data, C.byref(runs), C.byref(owner)))
    return vision._rle_records(offsets, runs, owner, n, w, h)


def host_loop_call(xy, poff, n, w, h):
    """the C call alone: the rows stay in the library's buffer and are released"""
    offsets, runs, owner = np.zeros(n + 1, np.int64), C.c_void_p(), C.c_void_p()
    L.check(L.get_lib().visp_image_rle_from_poly_reference_host(xy.ctypes.data, poff.ctypes.data, n, w, h, offsets.ctypes.data, C.byref(runs), C.byref(owner)))
    L.get_lib().visp_rle_destroy(owner)


def clock_ms(fn, samples, warmup):
    times = []
    for i in range(warmup + samples):
        t0 = time.perf_counter()
        fn()
        if i >= warmup:
            times.append((time.perf_counter() - t0) * 1e3)
    return stats(times)


def measure(api, polygons, w, h, samples, warmup, device):
    n, (xy, poff) = len(polygons), vision._polygon_rows(polygons)
    tv = int(poff[-1])
    want = host_loop(xy, poff, n, w, h)
    xd, pd, mkd, sd = U.dev(xy), U.dev(poff), U.empty(n * 16), U.empty(n * 4)
    ws0 = api.vx_poly_rle_workspace_bytes(tv, n, 0)
    w0 = U.empty(ws0)

    def sizing():
        L.vx_check(api.vx_poly_rle(xd.ptr, pd.ptr, tv, 0, n, w, h, None, 0, None, 0, None, None, None, mkd.ptr, None, w0.ptr, ws0, None))

    sizing()
    mk = mkd.to_numpy(np.int64, (n, 2))
    longest, total_keys = int(mk[:, 0].max()), sum(api.vx_poly_rle_key_row(int(k)) for k in mk[:, 1])
    ws = api.vx_poly_rle_workspace_bytes(tv, n, longest)
    wd, kd = U.empty(ws), U.empty(4 * total_keys + 16, zero=False)

    def count():
        L.vx_check(api.vx_poly_rle(xd.ptr, pd.ptr, tv, longest, n, w, h, None, 0, kd.ptr, total_keys, None, None, sd.ptr, None, None, wd.ptr, ws, None))

    count()
    offsets = np.concatenate([[0], np.cumsum(sd.to_numpy(np.int32, (n,)))]).astype(np.int64)
    rd, od = U.empty(4 * int(offsets[-1]) + 16, zero=False), U.dev(offsets)

    def write():
        L.vx_check(api.vx_poly_rle(xd.ptr, pd.ptr, tv, longest, n, w, h, None, 0, kd.ptr, total_keys, rd.ptr, od.ptr, None, None, None, wd.ptr, ws, None))

    write()
    U.sync()
    flat = np.array([c for r in want for c in r["counts"]], np.uint32)
    assert np.array_equal(rd.to_numpy(np.uint32, (int(offsets[-1]),)), flat), "the device's rows differ from the host loop's"
    return dict(polygons=n, vertices=tv, points_total=int(mk[:, 0].sum()), points_longest=longest, keys_total=int(mk[:, 1].sum()), keys_longest=int(mk[:, 1].max()),
                runs_total=int(offsets[-1]), sizing_ms=events_ms(sizing, samples, warmup), count_ms=events_ms(count, samples, warmup), write_ms=events_ms(write, samples, warmup),
                python_entry_ms=clock_ms(lambda: vision.poly_to_rle(polygons, h, w, device), samples, warmup),
                host_loop_ms=clock_ms(lambda: host_loop_call(xy, poff, n, w, h), samples, warmup))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--samples", type=int, default=7)
    ap.add_argument("--polygons", type=int, default=4000)
    ap.add_argument("--long-vertices", type=int, default=400)
    ap.add_argument("--out", default=str(Path(__file__).resolve().parents[1] / "profiles" / "mask_rle_poly_bench.txt"))
    a = ap.parse_args()
    api = U.api()
    assert api.vx_device_count() > 0, "no HIP device visible: there is nothing to measure without one"
    device = vision.Device.init(vision.Backend.gpu)
    coco = measure(api, coco_like(a.polygons, 640, 480), 640, 480, a.samples, a.warmup, device)
    print(f"COCO-like polygons at 640 x 480: {coco}")
    k = a.long_vertices
    outline = [np.array([(0.0 if j % 2 == 0 else 1024.0, (j + 0.5) * 1024 / k) for j in range(k)])]
    one_long = measure(api, outline, 1024, 1024, a.samples, a.warmup, device)
    print(f"one long outline at 1024 x 1024: {one_long}")
    U.release()
    line = json.dumps(dict(tool="bench_mask_rle_poly", coco_like=coco, one_long=one_long))
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(line + "\n")
    print(line)


if __name__ == "__main__":
    main()

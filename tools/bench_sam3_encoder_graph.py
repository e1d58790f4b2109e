#!/usr/bin/env python3
"""Timing of SAM3 vision-transformer layers built through the graph layer (vision.cpp_amd/graph.py::sam3_vision_layer) at SAM3's real dimensions -- hidden
1024, 16 heads of 64, MLP 4736, windows of 24 x 24 on a 72 x 72 token map, one image -- and of the rotation kernel behind them. Prints a text record and,
last, one JSON line. A measurement, not a gate.

  * `--layers N` layers (default 4: three window layers and one global layer, the pattern SAM3 repeats eight times) on synthetic weights, on a token map
    that is a graph input: launches per layer from the plan, and hipGraph-replay latency with fused models and with fused models off, the two graphs
    alternating in the same run: host clock around compute(), which ends in a stream synchronise; `samples` replays each after `warmup`; min / median / max
    and the ratio of the medians. The outputs of the two graphs are compared on the way.
  * kernel-only time of vx_rope2d_f16, in place on head-major q and k, at the window shape (B 9, T 576) and the global shape (B 1, T 5184), next to
    vx_copy_strided_f16 making the head-major copy of q and of k from token-major rows (what the per-node path runs besides): device events around `reps`
    back-to-back launches, `samples` windows per kernel after warm-up launches, the kernels alternating; GB/s from the bytes the pass must move (every
    element of q and k read once and written once; the rotation's tables, 2 x T x 32 f32, are not counted).

    python tools/bench_sam3_encoder_graph.py [--layers 4] [--samples 25] [--reps 20] [--warmup 5]"""
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
from tests import sam3_ref as R  # noqa: E402
from visioncpp_amd import _lib as L  # noqa: E402
from visioncpp_amd import graph as G  # noqa: E402
from visioncpp_amd import synth, vision  # noqa: E402

HIDDEN, HEADS, MLP, WINDOW, GRID, HD = 1024, 16, 4736, 24, 72, 64


def stats(ts):
    return dict(min=round(float(min(ts)), 2), median=round(float(np.median(ts)), 2), max=round(float(max(ts)), 2))


def window_us(fn, reps):
    api = U.api()
    e0, e1 = C.c_void_p(), C.c_void_p()
    api.vx_event_create(C.byref(e0)); api.vx_event_create(C.byref(e1))
    api.vx_event_record(e0, None)
    for _ in range(reps):
        fn()
    api.vx_event_record(e1, None)
    U.sync()
    ms = C.c_float()
    api.vx_event_elapsed_ms(e0, e1, C.byref(ms))
    api.vx_event_destroy(e0); api.vx_event_destroy(e1)
    return ms.value / reps * 1e3


def i64(v):
    return (C.c_int64 * len(v))(*[int(x) for x in v])


def bench_kernels(a):
    api = U.api()
    out = []
    for name, B, T, side, scale in [("window", (GRID // WINDOW) ** 2, WINDOW * WINDOW, WINDOW, 1.0), ("global", 1, GRID * GRID, GRID, WINDOW / GRID)]:
        rng = np.random.default_rng(T)
        px, py = R.rope_2d_positions(T, side)
        tx, ty = U.dev(R.rope_table(px, HD // 2, 10000.0, scale)), U.dev(R.rope_table(py, HD // 2, 10000.0, scale))
        q, k = (U.dev(rng.standard_normal((B, HEADS, T, HD)).astype(np.float16)) for _ in range(2))
        qt, kt = U.empty(B * HEADS * T * HD * 2), U.empty(B * HEADS * T * HD * 2)
        head = i64([HD * T, HD, HD * T * HEADS])
        ne, ss, ds = i64([HD, T, HEADS, B]), i64([1, HEADS * HD, HD, T * HEADS * HD]), i64([1, HD, T * HD, HEADS * T * HD])

        def rope():
            L.vx_check(api.vx_rope2d_f16(q.ptr, q.ptr, k.ptr, k.ptr, tx.ptr, ty.ptr, HD, HEADS, T, B, head, head, 1.0, None))

        def copies():  # heads_major of q and of k: two launches
            L.vx_check(api.vx_copy_strided_f16(q.ptr, qt.ptr, ne, ss, ds, 1.0, None))
            L.vx_check(api.vx_copy_strided_f16(k.ptr, kt.ptr, ne, ss, ds, 1.0, None))

        for _ in range(a.warmup):
            rope(); copies()
        U.sync()
        tr, tc = [], []
        for _ in range(a.samples):
            tr.append(window_us(rope, a.reps))
            tc.append(window_us(copies, a.reps))
        nbytes = 2 * B * HEADS * T * HD * 2 * 2  # q and k, read and written, f16
        row = dict(shape=name, B=B, heads=HEADS, T=T, hd=HD, bytes=nbytes, rope2d_us=stats(tr), rope2d_gbps=round(nbytes / np.median(tr) / 1e3, 1),
                   copy_strided_x2_us=stats(tc), copy_strided_gbps=round(nbytes / np.median(tc) / 1e3, 1))
        print(f"{name} shape (B {B}, heads {HEADS}, T {T}, hd {HD}; {nbytes / 1e6:.1f} MB moved): vx_rope2d_f16 in place on q and k {row['rope2d_us']} us = {row['rope2d_gbps']} GB/s;   "
              f"vx_copy_strided_f16 x 2 (heads_major q, k) {row['copy_strided_x2_us']} us = {row['copy_strided_gbps']} GB/s")
        out.append(row)
    return out


def bench_graph(a, device):
    cfg = synth.Sam3VitConfig(hidden=HIDDEN, heads=HEADS, mlp=MLP, patch=14, window=WINDOW, pretrain_grid=24, image_size=GRID * 14, n_layers=a.layers,
                              global_layers=tuple(range(3, a.layers, 4)), fpn_dim=256)
    t0 = time.perf_counter()
    sd = {k: v for k, v in synth.sam3_vision_state_dict(cfg, 0).items() if ".layers." in k}
    weights = G.Weights()
    for name, t in sd.items():
        weights.add(synth.sam3_tensor_name(name), t)
    print(f"{a.layers} layers of synthetic weights in {time.perf_counter() - t0:.1f} s; global layers {list(cfg.global_layers)}")
    x16 = np.random.default_rng(1).standard_normal((1, GRID, GRID, HIDDEN)).astype(np.float16)
    graphs, out = {}, {}
    for fused in (True, False):
        g = G.Graph(device, weights)
        g.set_fused_models(fused)
        m = G.ModelRef(g, "det.ve.backbone")
        x = g.input((HIDDEN, GRID, GRID, 1), G.F16, "tokens")
        pw = G.sam3_rope_2d_positions(m, WINDOW ** 2, WINDOW, 1.0, "_vit_rope_pos_window")
        pg = G.sam3_rope_2d_positions(m, GRID ** 2, GRID, WINDOW / GRID, "_vit_rope_pos_global")
        y = x
        for i in range(a.layers):
            glob = i in cfg.global_layers
            y = G.sam3_vision_layer(m["layers"][i], y, 0 if glob else WINDOW, HEADS, pg if glob else pw)
        y = g.output(y, "tokens_out")
        g.use_hip_graph(True)
        g.allocate()
        g.set(x, x16)
        for _ in range(a.warmup + 1):  # the first compute runs the launches one by one and records them
            g.compute()
        graphs["fused" if fused else "per_node"] = (g, y)
    ts = {k: [] for k in graphs}
    for _ in range(a.samples):
        for key, (g, _) in graphs.items():
            t0 = time.perf_counter()
            g.compute()
            ts[key].append((time.perf_counter() - t0) * 1e6)
    ya, yb = (graphs[k][0].get(graphs[k][1]) for k in ("fused", "per_node"))
    diff = float(np.abs(ya - yb).max() / np.abs(yb).max())
    for key, (g, _) in graphs.items():
        lines = g.describe().strip().splitlines()[:-1]
        out[key] = dict(launches=len(lines), launches_per_layer=round(len(lines) / a.layers, 2), rope_launches=sum(l.startswith("rope") for l in lines), replay_us=stats(ts[key]))
        print(f"{a.layers} layers ({key}): {out[key]['launches']} launches = {out[key]['launches_per_layer']} per layer, {out[key]['rope_launches']} of them rotations; "
              f"hipGraph replay {out[key]['replay_us']} us (host clock around compute(), {a.samples} replays, the two graphs alternating)")
    out["per_node_over_fused"] = round(out["per_node"]["replay_us"]["median"] / out["fused"]["replay_us"]["median"], 3)
    out["outputs_differ_by"] = float(f"{diff:.3g}")
    print(f"per node / fused (medians): {out['per_node_over_fused']}; the two outputs differ by {diff:.2e} of the largest value")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=4)
    ap.add_argument("--samples", type=int, default=25)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    if a.samples < 20:
        ap.error("--samples: at least 20")
    assert U.api().vx_device_count() > 0, "no HIP device visible: there is nothing to measure without one"
    device = vision.Device.init(vision.Backend.gpu)
    print(f"SAM3 vision layers through the graph layer: hidden {HIDDEN}, {HEADS} heads, MLP {MLP}, window {WINDOW}, {GRID} x {GRID} tokens; {a.samples} samples after "
          f"{a.warmup} warm-up rounds; kernel windows of {a.reps} launches")
    result = dict(tool="bench_sam3_encoder_graph", layers=a.layers, samples=a.samples, reps=a.reps, rope=bench_kernels(a), layers_graph=bench_graph(a, device))
    U.release()
    print(json.dumps(result))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Same-device timing of the two window-attention kernels on the same windows: vx_attention_masked_f16 (the graph layer's
ATTENTION_MASKED: head-major q / k / v, an additive f16 mask [Bm][heads][N][N] read per key block) against
vx_window_attention_masked_f16 (the hand schedule's: interleaved qkv rows, bias + shift mask pre-packed in accumulator order,
four window classes). Default shape = SWIN-T stage 0 at 1024 x 1024, batch 8: 256 x 256 tokens -> 37 x 37 windows of 7 x 7 per
image, 3 heads of 32. Device events around `reps` launches, three warm-up launches first, the two kernels alternating over
`rounds` rounds; the outputs are compared on the way. Prints a text record (profiles/): a measurement, not a gate.

    python tools/bench_window_attention.py [--batch 8] [--map 256] [--heads 3] [--ws 7] [--reps 20] [--rounds 5]"""
import argparse
import ctypes as C
import math
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from __graft_entry__ import load_package  # noqa: E402

load_package()
from tests import gpu_util as G  # noqa: E402
from visioncpp_amd import _lib as L  # noqa: E402
from visioncpp_amd import graph as GR  # noqa: E402


def timed(fn, reps):
    api = G.api()
    e0, e1 = C.c_void_p(), C.c_void_p()
    api.vx_event_create(C.byref(e0)); api.vx_event_create(C.byref(e1))
    for _ in range(3):
        fn()
    api.vx_event_record(e0, None)
    for _ in range(reps):
        fn()
    api.vx_event_record(e1, None)
    G.sync()
    ms = C.c_float()
    api.vx_event_elapsed_ms(e0, e1, C.byref(ms))
    api.vx_event_destroy(e0); api.vx_event_destroy(e1)
    return ms.value / reps * 1e3  # us per launch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--map", type=int, default=256, help="tokens per side of the stage's map (1024 / 4)")
    ap.add_argument("--heads", type=int, default=3)
    ap.add_argument("--ws", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    api = G.api()
    ws, heads, hd, N = a.ws, a.heads, 32, a.ws * a.ws
    nw_side = -(-a.map // ws)
    per_image, n_win = nw_side * nw_side, a.batch * nw_side * nw_side
    rng = np.random.default_rng(0)
    qkv = (rng.standard_normal((n_win * N, heads, 3, hd), dtype=np.float32) * 0.7).astype(np.float16)
    table = (rng.standard_normal(((2 * ws - 1) ** 2, heads)) * 0.5).astype(np.float32)

    # the packed-bias kernel's operands
    packed = np.zeros(4 * api.vx_window_attention_bias_bytes(N, heads) // 2, np.uint16)
    L.vx_check(api.vx_swin_attention_pack_bias(table.ctypes.data, ws, heads, packed.ctypes.data))
    d_qkv, d_packed = G.dev(qkv), G.dev(packed)
    out_a = G.empty(n_win * N * heads * hd * 2)

    # the masked kernel's operands: head-major q (scaled by log2(e) / sqrt(hd)), k, v; mask = bias[index] + shift mask, one image per window of a map
    r = qkv.reshape(n_win, N, heads, 3, hd)
    q = (r[:, :, :, 0].astype(np.float32) * (math.log2(math.e) / math.sqrt(hd))).astype(np.float16).transpose(0, 2, 1, 3)
    k, v = r[:, :, :, 1].transpose(0, 2, 1, 3), r[:, :, :, 2].transpose(0, 2, 1, 3)
    d_q, d_k, d_v = (G.dev(np.ascontiguousarray(t)) for t in (q, k, v))
    bias = table.astype(np.float16).astype(np.float32)[GR.swin_relative_position_index(ws).reshape(N, N)].transpose(2, 0, 1)  # [heads, query, key]
    mask = (bias[None] + GR.swin_attention_mask(a.map, a.map, ws)[:, None]).astype(np.float16)  # [per_image, heads, N, N]
    d_mask = G.dev(mask)
    d_mask_full = G.dev(np.ascontiguousarray(np.broadcast_to(mask[None], (a.batch,) + mask.shape)).reshape(n_win, heads, N, N))
    out_b = G.empty(n_win * N * heads * hd * 2)

    def run_packed():
        L.vx_check(api.vx_window_attention_masked_f16(d_qkv.ptr, d_packed.ptr, out_a.ptr, n_win, N, heads, nw_side, nw_side, None))

    def run_masked(m=d_mask, bm=per_image):
        L.vx_check(api.vx_attention_masked_f16(d_q.ptr, d_k.ptr, d_v.ptr, m.ptr, out_b.ptr, n_win, heads, N, hd, heads, bm, 0, None))

    run_packed(); run_masked(); G.sync()
    ya = out_a.to_numpy(np.float16, (n_win, N, heads * hd)).astype(np.float32)
    yb = out_b.to_numpy(np.float16, (n_win, N, heads * hd)).astype(np.float32)
    diff = float(np.abs(ya - yb).max() / np.abs(ya).max())

    rows = {"vx_window_attention_masked_f16 (packed bias, 4 classes)": run_packed,
            f"vx_attention_masked_f16 (mask [{per_image}][{heads}][{N}][{N}] f16, b % Bm)": run_masked,
            f"vx_attention_masked_f16 (mask repeated per image: Bm = {n_win})": lambda: run_masked(d_mask_full, n_win)}
    times = {name: [] for name in rows}
    for _ in range(a.rounds):
        for name, fn in rows.items():
            times[name].append(timed(fn, a.reps))
    flops = 4.0 * n_win * heads * N * N * hd
    print(f"window attention, SWIN stage: batch {a.batch}, map {a.map} x {a.map} tokens, window {ws}, {heads} heads of {hd}: {n_win} windows of {N} tokens")
    print(f"device events around {a.reps} launches after 3 warm-up launches, kernels alternating, {a.rounds} rounds; us per launch")
    print(f"outputs of the two kernels differ by {diff:.2e} of the largest value (f16 outputs)")
    for name, ts in times.items():
        med = float(np.median(ts))
        print(f"  {name:80s} median {med:8.1f} us  min {min(ts):8.1f}  max {max(ts):8.1f}   {flops / med / 1e6:6.1f} TFLOP/s (useful 4 N^2 hd per window-head)")
    base = float(np.median(times[list(rows)[0]]))
    for name in list(rows)[1:]:
        print(f"  ratio to the packed-bias kernel: {float(np.median(times[name])) / base:5.2f} x   <- {name}")
    G.release()


if __name__ == "__main__":
    main()

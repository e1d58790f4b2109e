#!/usr/bin/env python3
"""Same-device timing of the deformable convolution's two forms on the same operands: vx_deform_conv_f16 (the graph layer's fused group: an implicit
GEMM whose A loader samples, logits mode, batch-norm scale + bias + ReLU in the epilogue) against the composed form of csrc/birefnet.cpp
(vx_bf_deform_cols_f16 writes every sampled column to HBM, vx_gemm_f16 reads it back; batch norm folded into the weights, ReLU in the epilogue) --
the baseline. The offsets | logits product in front of both is the same launch and is not timed. Shapes: BiRefNet-lite's four decoder levels at
1024 x 1024, batch 8 (maps 32, 64, 128, 256 squared), Cin 64, Cout 256, kernels 1, 3, 7. Device events around `reps` launches after three warm-up
launches, the two forms alternating over `rounds` rounds; the outputs are compared on the way. Prints a text record and, last, one JSON line.
A measurement, not a gate. On a shared machine run it under a time limit of its own:

    timeout -k 10 900 python tools/bench_deform_conv.py [--batch 8] [--maps 32,64,128,256] [--kernels 1,3,7] [--reps 10] [--rounds 5]"""
import argparse
import ctypes as C
import json
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from __graft_entry__ import load_package  # noqa: E402

load_package()
from tests import gpu_util as G  # noqa: E402
from visioncpp_amd import _lib as L  # noqa: E402


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


def one_shape(B, side, k, cin, cout, reps, rounds):
    api = G.api()
    rng = np.random.default_rng(side + k)
    taps, M = k * k, B * side * side
    ldom = -(-3 * taps // 8) * 8
    x = rng.standard_normal((M, cin), dtype=np.float32).astype(np.float16)
    om = np.zeros((M, ldom), np.float16)
    om[:, :2 * taps] = (rng.standard_normal((M, 2 * taps), dtype=np.float32) * 0.6).astype(np.float16)  # offsets about half a pixel, as the model's
    om[:, 2 * taps:3 * taps] = rng.standard_normal((M, taps), dtype=np.float32).astype(np.float16)
    w = (rng.standard_normal((cout, taps * cin)) / np.sqrt(taps * cin)).astype(np.float32)
    scale = (1 + 0.1 * rng.standard_normal(cout)).astype(np.float32)
    bias = (0.1 * rng.standard_normal(cout)).astype(np.float32)
    d_x, d_om, d_scale, d_bias = G.dev(x), G.dev(om), G.dev(scale), G.dev(bias)
    d_w = G.dev(G.pad_weight(w, 32, 16))                      # fused: the kernel rows as they are
    w_folded = G.pad_weight(w * scale[:, None])               # composed: bn.weight folded in, K padded to 64 (csrc/birefnet.cpp:70)
    d_wf = G.dev(w_folded)
    cols = G.empty(M * taps * cin * 2 + 4096, zero=False)
    out_f, out_c = G.empty(M * cout * 2), G.empty(M * cout * 2)

    a = L.DeformConvArgs()
    a.x, a.B, a.H, a.W, a.Cin = d_x.ptr, B, side, side, cin
    a.w, a.Cout, a.k, a.pad = d_w.ptr, cout, k, k // 2
    a.offset, a.ld_offset, a.mask, a.ld_mask, a.mask_mode, a.mask_scale = d_om.ptr, ldom, d_om.ptr + 2 * taps * 2, ldom, 2, 2.0
    a.scale, a.bias, a.relu, a.out, a.ldo = d_scale.ptr, d_bias.ptr, 1, out_f.ptr, cout
    g = L.GemmArgs()
    g.A, g.lda, g.W, g.bias = cols.ptr, taps * cin, d_wf.ptr, d_bias.ptr
    g.M, g.N, g.K, g.epi, g.out, g.ldo, g.n_valid = M, w_folded.shape[0], w_folded.shape[1], L.EPI_F16_RELU, out_c.ptr, cout, cout

    def fused():
        L.vx_check(api.vx_deform_conv_f16(C.byref(a), None))

    def composed():
        L.vx_check(api.vx_bf_deform_cols_f16(d_x.ptr, d_om.ptr, ldom, cols.ptr, B, side, side, cin, k, None))
        L.vx_check(api.vx_gemm_f16(C.byref(g), None))

    def sample_only():
        L.vx_check(api.vx_bf_deform_cols_f16(d_x.ptr, d_om.ptr, ldom, cols.ptr, B, side, side, cin, k, None))

    fused(); composed(); G.sync()
    yf = out_f.to_numpy(np.float16, (M, cout)).astype(np.float32)
    yc = out_c.to_numpy(np.float16, (M, cout)).astype(np.float32)
    diff = float(np.abs(yf - yc).max() / np.abs(yc).max())
    t = {"fused": [], "composed": [], "cols": []}
    for _ in range(rounds):
        t["fused"].append(timed(fused, reps))
        t["composed"].append(timed(composed, reps))
        t["cols"].append(timed(sample_only, reps))
    G.release()
    med = {n: float(np.median(v)) for n, v in t.items()}
    flops = 2.0 * M * cout * taps * cin
    row = {"map": side, "k": k, "M": M, "K": taps * cin, "fused_us": round(med["fused"], 1), "composed_us": round(med["composed"], 1),
           "composed_cols_us": round(med["cols"], 1), "fused_min_us": round(min(t["fused"]), 1), "fused_max_us": round(max(t["fused"]), 1),
           "composed_min_us": round(min(t["composed"]), 1), "composed_max_us": round(max(t["composed"]), 1),
           "ratio_fused_over_composed": round(med["fused"] / med["composed"], 3), "fused_tflops": round(flops / med["fused"] / 1e6, 1),
           "cols_bytes": M * taps * cin * 2, "outputs_differ_by": diff}
    print(f"  map {side:3d}^2 k={k}: fused {med['fused']:9.1f} us ({row['fused_tflops']:6.1f} TFLOP/s)   composed {med['composed']:9.1f} us (sampling {med['cols']:8.1f} us, "
          f"{row['cols_bytes'] / 1e6:7.1f} MB of columns)   fused / composed {row['ratio_fused_over_composed']:5.2f}   outputs differ by {diff:.1e}", flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--maps", default="32,64,128,256")
    ap.add_argument("--kernels", default="1,3,7")
    ap.add_argument("--cin", type=int, default=64)
    ap.add_argument("--cout", type=int, default=256)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    assert G.api().vx_device_count() > 0, "no HIP device visible: a timing needs the GPU"
    print(f"deformable conv, fused (vx_deform_conv_f16) against composed (vx_bf_deform_cols_f16 + vx_gemm_f16): batch {a.batch}, Cin {a.cin}, Cout {a.cout}")
    print(f"device events around {a.reps} launches after 3 warm-up launches, forms alternating, {a.rounds} rounds; median us per call", flush=True)
    rows = [one_shape(a.batch, int(s), int(k), a.cin, a.cout, a.reps, a.rounds) for s in a.maps.split(",") for k in a.kernels.split(",")]
    print(json.dumps({"bench": "deform_conv_fused_vs_composed", "batch": a.batch, "cin": a.cin, "cout": a.cout, "reps": a.reps, "rounds": a.rounds, "shapes": rows}))


if __name__ == "__main__":
    main()

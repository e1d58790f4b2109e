#!/usr/bin/env python3
"""Timing of the SAM prompt encoder + mask decoder built through the graph layer (vision.cpp_amd/graph.py::sam_predict_mask), and of its attention kernel.
Prints a text record and, last, one JSON line. A measurement, not a gate.

  * hipGraph-replay latency of the full-size decoder graph (dim 256, mlp 2048, 64 x 64 embedding, one point prompt), fused and per node: host clock around
    compute(), which ends in a stream synchronise; `samples` replays after `warmup`, min / median / max; and the graph's launch count.
  * kernel-only time of vx_attention_cross_f16 at the decoder's three shapes (head_dim, heads, T_q, T_k) = (32, 8, 7, 7), (16, 8, 7, 4096), (16, 8, 4096, 7), and
    of the hand schedule's vx_small_attention_f16 on the same operands in the same run, the two alternating: device events around `reps` back-to-back
    launches, `samples` such windows per kernel after warm-up launches, min / median / max of the per-launch means. The outputs are compared on the way.
  * next to them, where the hand schedule can be built: wall time of visp_sam_compute (its whole call: prompt, decoder and mask post-processing) on a synthetic
    MobileSAM file, and its timing groups.

    python tools/bench_sam_decoder_graph.py [--samples 25] [--reps 20] [--warmup 5] [--skip-hand]"""
import argparse
import ctypes as C
import json
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from __graft_entry__ import load_package  # noqa: E402

load_package()
from tests import gpu_util as U  # noqa: E402
from visioncpp_amd import _lib as L  # noqa: E402
from visioncpp_amd import graph as G  # noqa: E402
from visioncpp_amd import synth, vision  # noqa: E402

SHAPES = [(32, 8, 7, 7), (16, 8, 7, 4096), (16, 8, 4096, 7)]


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


def bench_kernels(a):
    api = U.api()
    out = []
    for hd, H, Tq, Tk in SHAPES:
        rng = np.random.default_rng(hd + Tq)
        q = rng.standard_normal((Tq, H * hd)).astype(np.float16)
        k, v = rng.standard_normal((Tk, H * hd)).astype(np.float16), rng.standard_normal((Tk, H * hd)).astype(np.float16)
        dq, dk, dv = U.dev(q), U.dev(k), U.dev(v)
        oc, os_ = U.empty(Tq * H * hd * 2), U.empty(Tq * H * hd * 2)
        need = api.vx_attention_cross_partial_bytes(1, H, Tq, Tk, hd)
        part = U.empty(need) if need else None

        def cross():
            L.vx_check(api.vx_attention_cross_f16(dq.ptr, dk.ptr, dv.ptr, oc.ptr, part.ptr if part else None, need, 1, H, Tq, Tk, hd, hd ** -0.5, None))

        def small():
            L.vx_check(api.vx_small_attention_f16(dq.ptr, dk.ptr, dv.ptr, os_.ptr, Tq, Tk, H, hd, None))

        for _ in range(a.warmup):
            cross(); small()
        U.sync()
        yc, ys = (b.to_numpy(np.float16, (Tq, H * hd)).astype(np.float32) for b in (oc, os_))
        diff = float(np.abs(yc - ys).max() / np.abs(ys).max())
        tc, ts = [], []
        for _ in range(a.samples):
            tc.append(window_us(cross, a.reps))
            ts.append(window_us(small, a.reps))
        row = dict(hd=hd, heads=H, Tq=Tq, Tk=Tk, parts=api.vx_attention_cross_parts(Tq, Tk), cross_us=stats(tc), small_us=stats(ts), outputs_differ_by=float(f"{diff:.3g}"))
        print(f"attention (hd {hd}, heads {H}, T_q {Tq}, T_k {Tk}), parts {row['parts']}: vx_attention_cross_f16 {row['cross_us']} us   vx_small_attention_f16 {row['small_us']} us   "
              f"outputs differ by {diff:.2e} of the largest value")
        out.append(row)
    return out


def bench_graph(a, device):
    sd = synth.sam_decoder_state_dict(0)
    weights = G.Weights()
    for name, t in synth.sam_decoder_gguf_tensors(sd).items():
        weights.add(name, t.astype(np.float32), G.F32 if t.dtype == np.float32 else G.F16)
    embed = np.random.default_rng(1).standard_normal((64, 64, 256)).astype(np.float16)
    coords = np.array([[0.37, -0.41], [0.0, 0.0]], np.float32)
    out = {}
    for fused in (True, False):
        g = G.Graph(device, weights)
        g.set_fused_models(fused)
        m = G.ModelRef(g)
        ct, et = g.input((2, 2, 1), G.F32, "coords"), g.input((256, 64, 64, 1), G.F16, "embed")
        G.sam_predict_mask(m, et, G.sam_embed_points(m["prompt_encoder"], ct))
        g.use_hip_graph(True)
        g.allocate()
        g.set(ct, coords)
        g.set(et, embed)
        for _ in range(a.warmup + 1):  # the first compute runs the launches one by one and records them
            g.compute()
        ts = []
        for _ in range(a.samples):
            t0 = time.perf_counter()
            g.compute()
            ts.append((time.perf_counter() - t0) * 1e6)
        key = "fused" if fused else "per_node"
        out[key] = dict(launches=g.summary()["launches"], replay_us=stats(ts))
        print(f"decoder graph ({key}): {out[key]['launches']} launches, hipGraph replay {out[key]['replay_us']} us (host clock around compute(), {a.samples} replays)")
    return out


def bench_hand(a, device):
    with tempfile.TemporaryDirectory() as td:
        path = synth.write_mobile_sam_gguf(Path(td) / "mobile_sam.gguf", synth.TINYVIT_5M, seed=0)
        model = vision.Model.load(path, device)
        image = np.random.default_rng(2).integers(0, 256, (1024, 1024, 3), dtype=np.uint8)
        model.sam_encode(image)
        for _ in range(a.warmup):
            model.sam_compute([700, 300])
        ts = []
        for _ in range(a.samples):
            t0 = time.perf_counter()
            model.sam_compute([700, 300])
            ts.append((time.perf_counter() - t0) * 1e6)
        model.enable_timing(True)
        model.sam_compute([700, 300])
        groups = {t["name"]: round(t["ms"] * 1e3, 1) for t in model.read_timing()}
        print(f"hand schedule: visp_sam_compute (prompt + decoder + mask post-processing), wall {stats(ts)} us; timing groups of one call (us): {groups}")
        return dict(sam_compute_wall_us=stats(ts), timing_groups_us=groups)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=25)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--skip-hand", action="store_true")
    a = ap.parse_args()
    if a.samples < 20:
        ap.error("--samples: at least 20")
    assert U.api().vx_device_count() > 0, "no HIP device visible: there is nothing to measure without one"
    device = vision.Device.init(vision.Backend.gpu)
    print(f"SAM decoder through the graph layer; {a.samples} samples after {a.warmup} warm-up rounds; kernel windows of {a.reps} launches")
    result = dict(tool="bench_sam_decoder_graph", samples=a.samples, reps=a.reps, attention=bench_kernels(a), decoder_graph=bench_graph(a, device))
    if not a.skip_hand:
        try:
            result["hand_schedule"] = bench_hand(a, device)
        except Exception as e:  # the hand schedule's figure is a courtesy next to the graph's: say why it is missing
            result["hand_schedule"] = f"not measured: {e}"
            print("hand schedule:", result["hand_schedule"])
    U.release()
    print(json.dumps(result))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Same-device timing of the graph layer's MI-GAN path: vx_upfirdn2x_f16 (csrc/kernels_fir.hip) against the per-node chain it replaces, and migan_generate
built through the graph layer, fused and per node, next to the hand schedule's batch entry (csrc/migan.cpp) from the same run.

Kernel, at (h, C) = (128, 128) and (256, 64), batch 16: one vx_upfirdn2x_f16 launch against nearest x2 -> mul(plane) -> depthwise 4x4 pad 2 -> crop copy, four
launches on the same operands. Device events around `reps` launches after three warm-up launches, the two alternating over `rounds` rounds; median
microseconds and the run-to-run spread (max - min over the rounds). Next to each: the bytes the launch must move (input once, output once; for the chain
every intermediate written and read) and the time those bytes take at 6.3 TB/s, the HBM figure tools/bench_migan.py uses. The outputs (268 and 537 MB) exceed
the 256 MB Infinity Cache, so the launches of a round do not find their operands there.

Network, res 512, batch 16, synthetic weights: the graph fused and per node, each replayed as one hipGraph (the f32 image on the device): a host clock around
`steps` computes that end in a device synchronise, after three warm-up computes. The hand schedule: visp_migan_compute_batch_device on u8 images (its
preprocess and u8 postprocess included), the same clock. Not the same work at the two ends, so the tool forms no ratio of them.

Prints a text record and, last, one JSON line. A measurement, not a gate. On a shared machine run it under a time limit of its own:

    timeout -k 10 600 python tools/bench_migan_graph.py [--batch 16] [--res 512] [--steps 30] [--reps 20] [--rounds 5]"""
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
from tests import gpu_util as G  # noqa: E402
from visioncpp_amd import _lib as L  # noqa: E402
from visioncpp_amd import graph as GR  # noqa: E402
from visioncpp_amd import synth, vision  # noqa: E402

HBM = 6.3e12


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
    return ms.value / reps * 1e3  # us per repetition


def upfir_case(B, h, Cc, reps, rounds):
    api = G.api()
    rng = np.random.default_rng(h + Cc)
    x = G.dev(rng.standard_normal((B, h, h, Cc), dtype=np.float32).astype(np.float16))
    fir = np.outer([1.0, 3.0, 3.0, 1.0], [1.0, 3.0, 3.0, 1.0]) / 16.0
    f = G.dev(np.repeat(fir.reshape(16, 1), Cc, 1).astype(np.float16))
    tile = G.dev(np.tile(np.array([[1.0, 0.0], [0.0, 0.0]], np.float32), (h, h)))
    H2 = 2 * h
    n_in, n_up, n_pad = B * h * h * Cc, B * H2 * H2 * Cc, B * (H2 + 1) * (H2 + 1) * Cc
    y_f, y_c, up, masked, padded = G.empty(n_up * 2), G.empty(n_up * 2), G.empty(n_up * 2), G.empty(n_up * 2), G.empty(n_pad * 2)
    ne = (C.c_int64 * 4)(Cc, H2, H2, B)
    ss = (C.c_int64 * 4)(1, Cc, Cc * (H2 + 1), Cc * (H2 + 1) * (H2 + 1))
    ds = (C.c_int64 * 4)(1, Cc, Cc * H2, Cc * H2 * H2)

    def fused():
        L.vx_check(api.vx_upfirdn2x_f16(x.ptr, Cc, f.ptr, y_f.ptr, Cc, None, None, 0, 0, 1.0, 0.0, B, h, h, Cc, None))

    def chain():
        L.vx_check(api.vx_nearest_f16(x.ptr, up.ptr, B, h, h, Cc, H2, H2, None))
        L.vx_check(api.vx_binary_plane_f16(1, up.ptr, tile.ptr, 1, masked.ptr, B, H2 * H2, Cc, None))
        L.vx_check(api.vx_dwconv_f16(masked.ptr, f.ptr, None, padded.ptr, B, H2, H2, Cc, 4, 1, 2, 0, 0.0, None))
        L.vx_check(api.vx_copy_strided_f16(padded.ptr, y_c.ptr, ne, ss, ds, 1.0, None))

    fused(); chain(); G.sync()
    same = np.array_equal(y_f.to_numpy(np.float16, (n_up,)), y_c.to_numpy(np.float16, (n_up,)))
    t = {"fused": [], "chain": []}
    for _ in range(rounds):
        t["fused"].append(timed(fused, reps))
        t["chain"].append(timed(chain, reps))
    G.release()
    b_fused, b_chain = (n_in + n_up) * 2, (n_in + n_up + 2 * n_up + n_up + n_pad + n_pad + n_up) * 2
    row = {"case": f"B={B} {h}^2 x {Cc}", "upfirdn_us": round(float(np.median(t["fused"])), 1), "upfirdn_spread_us": round(max(t["fused"]) - min(t["fused"]), 1),
           "chain_us": round(float(np.median(t["chain"])), 1), "chain_spread_us": round(max(t["chain"]) - min(t["chain"]), 1), "same_bits": bool(same),
           "upfirdn_bytes": b_fused, "upfirdn_byte_bound_us": round(b_fused / HBM * 1e6, 1), "chain_bytes": b_chain, "chain_byte_bound_us": round(b_chain / HBM * 1e6, 1)}
    print(f"  {row['case']:18s} upfirdn2x {row['upfirdn_us']:8.1f} us (spread {row['upfirdn_spread_us']:6.1f}, byte bound {row['upfirdn_byte_bound_us']:7.1f})   "
          f"per-node chain {row['chain_us']:8.1f} us (spread {row['chain_spread_us']:6.1f}, byte bound {row['chain_byte_bound_us']:7.1f})   same bits: {same}", flush=True)
    return row


def network(batch, res, steps):
    rec = {"batch": batch, "res": res, "steps": steps}
    with tempfile.TemporaryDirectory() as td:
        path = synth.write_migan_gguf(Path(td) / "m.gguf", res, seed=1)
        dev = vision.Device.init(vision.Backend.gpu)
        x4 = np.random.default_rng(2).uniform(-1, 1, (batch, res, res, 4)).astype(np.float32)
        for fused in (True, False):
            g = GR.Graph(dev, GR.Weights(path))
            image = g.input((4, res, res, batch), GR.F32, "image")
            GR.migan_generate(GR.ModelRef(g), image, res)
            g.set_fused_models(fused)
            g.use_hip_graph(True)
            g.allocate()
            g.set(image, x4)
            for _ in range(3):
                g.compute()
            t0 = time.perf_counter()
            for _ in range(steps):
                g.compute()
            dt = (time.perf_counter() - t0) / steps
            key = "fused" if fused else "per_node"
            rec[f"graph_{key}_launches"] = g.summary()["launches"]
            rec[f"graph_{key}_ms"] = round(dt * 1e3, 3)
            rec[f"graph_{key}_images_per_s"] = round(batch / dt, 1)
            print(f"  graph-built, {key}: {rec[f'graph_{key}_launches']} launches, {rec[f'graph_{key}_ms']} ms = {rec[f'graph_{key}_images_per_s']} images / s", flush=True)
            del g
        model = vision.Migan.load(path, dev)
        imgs = synth.images(batch, res, res, seed=3)
        masks = np.zeros((batch, res, res), np.uint8)
        masks[:, res // 4:res // 2, res // 3:2 * res // 3] = 255
        din, dmask, dout = vision.DeviceBuffer.from_numpy(imgs), vision.DeviceBuffer.from_numpy(masks), vision.DeviceBuffer(batch * res * res * 4)
        run = lambda: L.check(G.api().visp_migan_compute_batch_device(model._handle, din.ptr, 3, dmask.ptr, batch, dout.ptr, None))  # noqa: E731
        for _ in range(3):
            run()
        t0 = time.perf_counter()
        for _ in range(steps):
            run()
        dt = (time.perf_counter() - t0) / steps
        rec["hand_batch_ms"] = round(dt * 1e3, 3)
        rec["hand_images_per_s"] = round(batch / dt, 1)
        print(f"  hand schedule (visp_migan_compute_batch_device: u8 in, u8 out; other work at the two ends: no ratio): {rec['hand_batch_ms']} ms = {rec['hand_images_per_s']} images / s", flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    assert G.api().vx_device_count() > 0, "no HIP device visible: a timing needs the GPU"
    print(f"vx_upfirdn2x_f16 against nearest -> mul_plane -> dwconv4x4 -> crop: batch {a.batch}; device events around {a.reps} launches after 3 warm-up launches, {a.rounds} rounds; "
          f"median us, spread = max - min over rounds; byte bound at {HBM / 1e12} TB/s", flush=True)
    kernels = [upfir_case(a.batch, h, c, a.reps, a.rounds) for h, c in ((128, 128), (256, 64))]
    print(f"MI-GAN at res {a.res}, batch {a.batch}: graph-built generator replayed as a hipGraph and the hand schedule's batch entry (host clock around {a.steps} calls)", flush=True)
    print(json.dumps({"bench": "migan_graph", "reps": a.reps, "rounds": a.rounds, "kernels": kernels, "network": network(a.batch, a.res, a.steps)}))


if __name__ == "__main__":
    main()

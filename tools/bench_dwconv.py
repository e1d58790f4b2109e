#!/usr/bin/env python3
"""Same-device timing of the graph layer's generic depthwise kernel (vx_dwconv_f16, csrc/kernels_dwconv.hip; k 3, pad 1) against the hand schedule's
3x3 kernel (vx_dwconv3x3_f16, csrc/kernels_tinyvit.hip) on the same operands, at the depthwise shapes of TinyViT-5M at 1024 x 1024, batch 16: maps
256^2 x 256 (stride 1), 256^2 x 128 (stride 2), 128^2 x 128 (1), 128^2 x 160 (2), 64^2 x 160 (1), 64^2 x 320 (1); bias and GELU on in both. Device events
around `reps` launches after three warm-up launches, the two kernels alternating over `rounds` rounds; median microseconds per launch, the run-to-run
spread (max - min over the rounds) of each, and achieved GB/s against the algorithmic bytes (input + output + kernel, each once). The outputs are
compared on the way.

With --encoder it also reports images / s of the TinyViT-5M encoder built through graph.tinyvit_encode (fused models, hipGraph replay, the f32 image on
the device) next to the hand schedule's visp_sam_encode_batch_device on the same weights: a host clock around `steps` calls that end in a device
synchronise, after two warm-up calls.

Prints a text record and, last, one JSON line. A measurement, not a gate. On a shared machine run it under a time limit of its own:

    timeout -k 10 600 python tools/bench_dwconv.py [--batch 16] [--reps 100] [--rounds 7] [--encoder] [--steps 50]"""
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

SHAPES = [(256, 256, 1), (256, 128, 2), (128, 128, 1), (128, 160, 2), (64, 160, 1), (64, 320, 1)]  # (map side, channels, stride)


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


def one_shape(B, side, Cc, stride, reps, rounds):
    api = G.api()
    rng = np.random.default_rng(side + Cc)
    out_side = (side + 2 - 3) // stride + 1
    x = rng.standard_normal((B * side * side, Cc), dtype=np.float32).astype(np.float16)
    w = (rng.standard_normal((9, Cc), dtype=np.float32) / 3).astype(np.float16)
    bias = (0.1 * rng.standard_normal(Cc)).astype(np.float32)
    d_x, d_w, d_b = G.dev(x), G.dev(w), G.dev(bias)
    n_out = B * out_side * out_side * Cc
    y_g, y_h = G.empty(n_out * 2), G.empty(n_out * 2)

    def generic():
        L.vx_check(api.vx_dwconv_f16(d_x.ptr, d_w.ptr, d_b.ptr, y_g.ptr, B, side, side, Cc, 3, stride, 1, 1, 0.0, None))

    def hand():
        L.vx_check(api.vx_dwconv3x3_f16(d_x.ptr, d_w.ptr, d_b.ptr, y_h.ptr, B, side, side, Cc, stride, 1, None))

    generic(); hand(); G.sync()
    a, b = y_g.to_numpy(np.float16, (n_out,)).astype(np.float32), y_h.to_numpy(np.float16, (n_out,)).astype(np.float32)
    diff = float(np.abs(a - b).max() / np.abs(b).max())
    t = {"generic": [], "hand": []}
    for _ in range(rounds):
        t["generic"].append(timed(generic, reps))
        t["hand"].append(timed(hand, reps))
    G.release()
    med = {n: float(np.median(v)) for n, v in t.items()}
    spread = {n: float(max(v) - min(v)) for n, v in t.items()}
    nbytes = (x.size + n_out + w.size) * 2 + bias.size * 4
    row = {"map": side, "C": Cc, "stride": stride, "generic_us": round(med["generic"], 1), "hand3x3_us": round(med["hand"], 1), "generic_spread_us": round(spread["generic"], 1),
           "hand3x3_spread_us": round(spread["hand"], 1), "generic_minus_hand_us": round(med["generic"] - med["hand"], 1),
           "slower_by_more_than_twice_the_spread": bool(med["generic"] - med["hand"] > 2 * spread["hand"]), "ratio_generic_over_hand": round(med["generic"] / med["hand"], 3),
           "bytes": nbytes, "generic_gbs": round(nbytes / med["generic"] / 1e3, 0), "hand3x3_gbs": round(nbytes / med["hand"] / 1e3, 0), "outputs_differ_by": diff}
    print(f"  {side:3d}^2 x {Cc:3d} s{stride}: generic {med['generic']:8.1f} us ({row['generic_gbs']:6.0f} GB/s, spread {spread['generic']:6.1f})   3x3 kernel {med['hand']:8.1f} us "
          f"({row['hand3x3_gbs']:6.0f} GB/s, spread {spread['hand']:6.1f})   generic / 3x3 {row['ratio_generic_over_hand']:5.3f}   outputs differ by {diff:.1e}", flush=True)
    return row


def encoder(batch, steps):
    """images / s of the graph-built TinyViT-5M encoder and of the hand schedule, device-resident inputs, the same synthetic weights"""
    from visioncpp_amd import graph as GR
    from visioncpp_amd import synth, vision
    cfg = synth.TINYVIT_5M
    with tempfile.TemporaryDirectory() as td:
        path = synth.write_tinyvit_gguf(Path(td) / "tinyvit_5m.gguf", cfg, seed=0)
        dev = vision.Device.init(vision.Backend.gpu)
        g = GR.Graph(dev, GR.Weights(path))
        image = g.input((3, cfg.img_size, cfg.img_size, batch), GR.F32, "image")
        g.output(GR.tinyvit_encode(GR.ModelRef(g, "enc"), image, cfg.layers()), "out")
        g.use_hip_graph(True)
        g.allocate()
        launches = g.summary()["launches"]
        imgs = synth.images(batch, cfg.img_size, cfg.img_size, seed=7)
        mean, std = np.array([0.485, 0.456, 0.406], np.float32), np.array([0.229, 0.224, 0.225], np.float32)
        g.set(image, ((imgs.astype(np.float32) / np.float32(255.0) - mean) / std).astype(np.float32))

        def clock(fn):
            for _ in range(2):
                fn()
            G.sync()
            t0 = time.perf_counter()
            for _ in range(steps):
                fn()
            G.sync()
            return (time.perf_counter() - t0) / steps

        t_graph = clock(g.compute)
        model = vision.Model.load(path, dev)
        rgb, out = G.dev(imgs), G.empty(batch * 64 * 64 * 256 * 4)
        t_hand = clock(lambda: model.sam_encode_batch_device(rgb.ptr, batch, out.ptr))
        G.release()
    row = {"batch": batch, "steps": steps, "graph_launches": launches, "graph_ms": round(t_graph * 1e3, 2), "hand_ms": round(t_hand * 1e3, 2),
           "graph_images_per_s": round(batch / t_graph, 1), "hand_images_per_s": round(batch / t_hand, 1)}
    print(f"  TinyViT-5M encoder, 1024^2, batch {batch}: graph-built (fused, {launches} launches) {row['graph_ms']} ms = {row['graph_images_per_s']} images / s;   "
          f"hand schedule (sam_encode_batch_device, u8 image in) {row['hand_ms']} ms = {row['hand_images_per_s']} images / s", flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--encoder", action="store_true")
    ap.add_argument("--steps", type=int, default=50)
    a = ap.parse_args()
    assert G.api().vx_device_count() > 0, "no HIP device visible: a timing needs the GPU"
    print(f"depthwise 3x3 pad 1 + bias + GELU, generic (vx_dwconv_f16) against the hand schedule's kernel (vx_dwconv3x3_f16): batch {a.batch}")
    print(f"device events around {a.reps} launches after 3 warm-up launches, kernels alternating, {a.rounds} rounds; median us per launch, spread = max - min over rounds", flush=True)
    rows = [one_shape(a.batch, s, c, st, a.reps, a.rounds) for s, c, st in SHAPES]
    rec = {"bench": "dwconv_generic_vs_3x3", "batch": a.batch, "reps": a.reps, "rounds": a.rounds, "shapes": rows}
    if a.encoder:
        rec["encoder"] = encoder(a.batch, a.steps)
    print(json.dumps(rec))


if __name__ == "__main__":
    main()

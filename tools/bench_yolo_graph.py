#!/usr/bin/env python3
"""Same-device timing of YOLOv9t built through the graph layer (graph.yolov9t_forward) against the hand schedule (csrc/yolov9t.cpp), and of the generic
pool kernel (vx_pool2d_f16, csrc/kernels_pool.hip) against the hand schedule's two special kernels on the same operands.

Network: S = 640, batch 16, synthetic weights; the graph with fused models and per node, each replayed as one hipGraph (the f32 image on the device): a
host clock around `steps` computes that end in a device synchronise, after three warm-up computes (the second of which captures). Next to it the device
time of the hand schedule's replayed launch list for the same batch (visp_yolov9t_last_split's device_ms, HIP events), which covers the u8 preprocess
and the decode with its candidate list as well; its readback and NMS are not counted on either side. The two figures are not the same work and
not the same clock, so the tool forms no ratio of them.

Pools, at the network's shapes at S = 640, batch 16: SPPELAN's three chained 5x5 / s1 / p2 maxima as three generic launches against the one
vx_yolo_spp_f16 launch (20^2 x 64 inside the 256-channel concat buffer), and AConv's 2x2 / s1 average against vx_yolo_avgpool2_f16 at the three
distinct AConv input shapes (160^2 x 32, 80^2 x 64, 40^2 x 96). Device events around `reps` launches after three warm-up launches, the kernels alternating over `rounds` rounds; median microseconds, the
run-to-run spread (max - min over the rounds) of each, and whether the outputs are the same bits. The launches of a round run back to back on one set of
buffers of 3 to 26 MB, which stay cache resident: these are not times from HBM.

Prints a text record and, last, one JSON line. A measurement, not a gate. On a shared machine run it under a time limit of its own:

    timeout -k 10 600 python tools/bench_yolo_graph.py [--batch 16] [--size 640] [--steps 200] [--reps 100] [--rounds 7]"""
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


def alternate(fns: dict, reps, rounds):
    t = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            t[k].append(timed(fn, reps))
    return {k: float(np.median(v)) for k, v in t.items()}, {k: float(max(v) - min(v)) for k, v in t.items()}


def pool_row(name, med, spread, same_bits):
    gain = med["generic"] - med["special"]
    row = {"case": name, "generic_us": round(med["generic"], 1), "special_us": round(med["special"], 1), "generic_spread_us": round(spread["generic"], 1),
           "special_spread_us": round(spread["special"], 1), "ratio_generic_over_special": round(med["generic"] / med["special"], 3), "same_bits": bool(same_bits),
           "special_faster_by_more_than_twice_its_spread": bool(gain > 2 * spread["special"])}
    print(f"  {name:28s} generic {med['generic']:8.1f} us (spread {spread['generic']:6.1f})   special {med['special']:8.1f} us (spread {spread['special']:6.1f})   "
          f"generic / special {row['ratio_generic_over_special']:5.3f}   same bits: {same_bits}", flush=True)
    return row


def spp_case(B, side, Cc, reps, rounds):
    api = G.api()
    x = np.zeros((B, side, side, 4 * Cc), np.float16)
    x[..., :Cc] = np.random.default_rng(1).standard_normal((B, side, side, Cc), dtype=np.float32).astype(np.float16)
    a, b = G.dev(x), G.dev(x)

    def generic():
        for i in range(3):
            L.vx_check(api.vx_pool2d_f16(a.ptr + i * Cc * 2, 4 * Cc, a.ptr + (i + 1) * Cc * 2, 4 * Cc, B, side, side, Cc, 0, 5, 1, 2, None))

    def special():
        L.vx_check(api.vx_yolo_spp_f16(b.ptr, 4 * Cc, B, side, side, Cc, None))

    generic(); special(); G.sync()
    same = np.array_equal(a.to_numpy(np.float16, x.shape), b.to_numpy(np.float16, x.shape))
    med, spread = alternate({"generic": generic, "special": special}, reps, rounds)
    G.release()
    return pool_row(f"spp 3 x max5x5 {side}^2 x {Cc}", med, spread, same)


def avg_case(B, side, Cc, reps, rounds):
    api = G.api()
    x = np.random.default_rng(side + Cc).standard_normal((B, side, side, Cc), dtype=np.float32).astype(np.float16)
    d_x = G.dev(x)
    n_out = B * (side - 1) * (side - 1) * Cc
    y_g, y_s = G.empty(n_out * 2), G.empty(n_out * 2)

    def generic():
        L.vx_check(api.vx_pool2d_f16(d_x.ptr, Cc, y_g.ptr, Cc, B, side, side, Cc, 1, 2, 1, 0, None))

    def special():
        L.vx_check(api.vx_yolo_avgpool2_f16(d_x.ptr, Cc, y_s.ptr, B, side, side, Cc, None))

    generic(); special(); G.sync()
    same = np.array_equal(y_g.to_numpy(np.float16, (n_out,)), y_s.to_numpy(np.float16, (n_out,)))
    med, spread = alternate({"generic": generic, "special": special}, reps, rounds)
    G.release()
    return pool_row(f"avg2x2 s1 {side}^2 x {Cc}", med, spread, same)


def network(batch, size, steps):
    rec = {"batch": batch, "size": size, "steps": steps}
    with tempfile.TemporaryDirectory() as td:
        path = synth.write_yolov9t_gguf(Path(td) / "y.gguf", seed=0)
        dev = vision.Device.init(vision.Backend.gpu)
        imgs = synth.images(batch, size, size, seed=3)
        for fused in (True, False):
            g = GR.Graph(dev, GR.Weights(path))
            image = g.input((3, size, size, batch), GR.F32, "image")
            boxes, scores, raw, _ = GR.yolov9t_forward(GR.ModelRef(g), image)
            g.output(boxes, "boxes"); g.output(scores, "scores")
            g.set_fused_models(fused)
            g.use_hip_graph(True)
            g.allocate()
            g.set(image, imgs.astype(np.float32) / np.float32(255.0))
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
        model = vision.Yolov9t.load(path, dev)
        for _ in range(3):
            model.detect_batch(imgs)
        dev_ms = []
        for _ in range(steps):
            model.detect_batch(imgs)
            dev_ms.append(model.last_split["device_ms"])
        rec["hand_device_ms"] = round(float(np.median(dev_ms)), 3)
        rec["hand_images_per_s_device"] = round(batch / (rec["hand_device_ms"] / 1e3), 1)
        print(f"  hand schedule (detect_batch, device time of the replayed launch list; other work, other clock: no ratio): {rec['hand_device_ms']} ms = "
              f"{rec['hand_images_per_s_device']} images / s", flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--size", type=int, default=640)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=7)
    a = ap.parse_args()
    assert G.api().vx_device_count() > 0, "no HIP device visible: a timing needs the GPU"
    s = a.size
    print(f"generic pool kernel (vx_pool2d_f16) against vx_yolo_spp_f16 / vx_yolo_avgpool2_f16: batch {a.batch}, the shapes of YOLOv9t at S = {s}")
    print(f"device events around {a.reps} launches after 3 warm-up launches, kernels alternating, {a.rounds} rounds; median us, spread = max - min over rounds", flush=True)
    pools = [spp_case(a.batch, s // 32, 64, a.reps, a.rounds)]
    pools += [avg_case(a.batch, side, c, a.reps, a.rounds) for side, c in ((s // 4, 32), (s // 8, 64), (s // 16, 96))]
    print(f"YOLOv9t at S = {s}, batch {a.batch}: graph-built network replayed as a hipGraph (host clock around {a.steps} computes) and the hand schedule's device time", flush=True)
    rec = {"bench": "yolov9t_graph", "reps": a.reps, "rounds": a.rounds, "pools": pools, "network": network(a.batch, a.size, a.steps)}
    print(json.dumps(rec))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Depth-Anything-V2 Small / Base / Large throughput at 518 x 518 on one GPU (synthetic weights of each checkpoint's shapes), one JSON
line per variant: images/s and ms per step of the replayed step (inputs resident in HBM, hipGraph replay on a non-null stream), the
timing table's FLOPs per image, the TFLOP/s that gives and its fraction of the dense f16 MFMA peak, and the per-kernel-group times of
direct launches. Batch 32 for Small and Base; Large takes the largest of 32 / 16 / 8 that the device accepts (stated in the line).
bench.py stays the measure of the flagship (Small) workload."""
import argparse
import gc
import json
import sys
import tempfile
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from __graft_entry__ import load_package  # noqa: E402

load_package()
import numpy as np  # noqa: E402
import torch  # noqa: E402

from visioncpp_amd import _lib as L  # noqa: E402
from visioncpp_amd import synth, vision  # noqa: E402

PEAK_MFMA_F16 = 2.5e15  # MI355X dense f16 MFMA
S = 518

ap = argparse.ArgumentParser()
ap.add_argument("--variants", default="small,base,large")
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
a = ap.parse_args()
CFGS = {"small": (synth.SMALL, (32,)), "base": (synth.BASE, (32,)), "large": (synth.LARGE, (32, 16, 8))}
dev = vision.Device.init(vision.Backend.gpu)
stream = torch.cuda.Stream()  # a real stream: required for hipGraph capture

for name in a.variants.split(","):
    cfg, batches = CFGS[name]
    with tempfile.TemporaryDirectory() as td:
        model = vision.Model.load(synth.write_gguf(Path(td) / f"{name}.gguf", cfg, seed=0), dev)
    B = None
    for b in batches:
        try:
            model.reserve(b, S, S)
            B = b
            break
        except L.Error as e:
            print(f"{name}: batch {b} refused: {e}", file=sys.stderr)
    assert B is not None, f"{name}: no batch fits"
    imgs = synth.images(8, S, S, seed=1234)
    imgs = np.concatenate([imgs] * (B // 8))
    rgb = torch.from_numpy(imgs).cuda()
    out = torch.empty((B, S, S), dtype=torch.float32, device="cuda")

    def step():
        model.compute_batch_device(rgb.data_ptr(), B, S, S, out.data_ptr(), None, stream.cuda_stream)

    # per-kernel-group table of direct launches (untimed region)
    step()
    torch.cuda.synchronize()
    model.enable_timing(True)
    acc: dict[str, dict] = {}
    reps = 3
    for _ in range(reps):
        step()
        torch.cuda.synchronize()
        for t in model.read_timing():
            g = acc.setdefault(t["name"], dict(ms=0.0, flops=0.0, launches=0))
            g["ms"] += t["ms"] / reps
            g["flops"] = t["flops"]
            g["launches"] = t["launches"]
    model.enable_timing(False)
    # timed region: hipGraph replay
    model.use_graph(True)
    for _ in range(a.warmup):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        step()
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / a.steps
    model.use_graph(False)
    o = out.cpu().numpy()
    assert np.isfinite(o).all() and o.min() >= 0 and o.max() <= 1 + 1e-6, "invalid output"
    groups = sorted(((k, v) for k, v in acc.items() if not k.startswith("__")), key=lambda kv: -kv[1]["ms"])
    flops = sum(v["flops"] for _, v in groups)
    ips = B / dt
    tflops = ips * flops / B / 1e12
    res = dict(variant=name, extent=[S, S], batch=B, embed_dim=cfg.embed_dim, n_layers=cfg.n_layers, steps=a.steps, warmup=a.warmup,
               images_per_s=round(ips, 2), ms_per_step=round(dt * 1e3, 3), gflop_per_image=round(flops / B / 1e9, 2),
               tflops=round(tflops, 2), mfma_peak_frac=round(tflops * 1e12 / PEAK_MFMA_F16, 4),
               launches_per_step=int(sum(v["launches"] for _, v in groups)),
               kernel_groups_ms={k: round(v["ms"], 3) for k, v in groups})
    if name == "large":
        res["batch_note"] = f"largest of {list(batches)} the device accepted"
    print(json.dumps(res), flush=True)
    del model, rgb, out
    gc.collect()
    torch.cuda.empty_cache()

#!/usr/bin/env python3
"""YOLOv9t throughput on one GPU (synthetic weights of the real channel table), one JSON line:
batch-1 detect latency from a 1280x720 host image, images/s at batch 1, 16 and 64 with each call split into the replayed launch
list's device time (HIP events), the candidate readback and the host NMS, the
schedule's own GFLOP / bytes per image and the share of the HBM or MFMA bound (whichever binds)."""
import argparse
import json
import sys
import tempfile
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from __graft_entry__ import load_package  # noqa: E402

load_package()
import numpy as np  # noqa: E402

from visioncpp_amd import synth, vision  # noqa: E402

HBM_BPS, MFMA_FLOPS = 8.0e12, 2.5e15  # MI355X: HBM3E bandwidth, dense f16 MFMA peak

ap = argparse.ArgumentParser()
ap.add_argument("--size", type=int, default=640)
ap.add_argument("--iters", type=int, default=20)
a = ap.parse_args()
S = a.size
dev = vision.Device.init(vision.Backend.gpu)
with tempfile.TemporaryDirectory() as td:
    model = vision.Yolov9t.load(synth.write_yolov9t_gguf(Path(td) / "y.gguf", seed=0), dev)
img = synth.images(1, 1280, 720, seed=1)[0]
for _ in range(3):
    model.detect(img)
t = time.perf_counter()
for _ in range(a.iters):
    dets = model.detect(img)
lat_ms = (time.perf_counter() - t) / a.iters * 1e3
res = dict(model="yolov9t", size=S, detect_1280x720_ms=round(lat_ms, 3), detections=int(len(dets)))
model.enable_timing(True)
model.detect_batch(synth.images(1, S, S, seed=2))
rows = model.read_timing()
model.enable_timing(False)
flops, byts = sum(r["flops"] for r in rows), sum(r["bytes"] for r in rows)
res["gflop_per_image"] = round(flops / 1e9, 3)
res["mbytes_per_image"] = round(byts / 1e6, 2)
res["groups_ms_b1"] = {r["name"]: round(r["ms"], 4) for r in rows}
for B in (1, 16, 64):
    imgs = synth.images(B, S, S, seed=3)
    for _ in range(3):
        model.detect_batch(imgs)  # eager warm-up, capture, replay
    n = max(3, a.iters // (1 if B == 1 else 4))
    t = time.perf_counter()
    for _ in range(n):
        model.detect_batch(imgs)
    dt = (time.perf_counter() - t) / n
    sp = model.last_split  # the last replayed call: launch list on the device (HIP events), candidate readback, host NMS
    res[f"batch{B}_split_ms"] = {k: round(v, 3) for k, v in sp.items()}
    res[f"batch{B}_ms"] = round(dt * 1e3, 3)
    res[f"batch{B}_images_per_s"] = round(B / dt, 1)
    if B == 64:
        model.enable_timing(True)
        model.detect_batch(imgs)
        rows = model.read_timing()
        model.enable_timing(False)
        dev_ms = sum(r["ms"] for r in rows)
        res["batch64_device_ms_eager"] = round(dev_ms, 3)
        res["batch64_groups_ms"] = {r["name"]: round(r["ms"], 3) for r in rows}
        t_hbm, t_mfma = byts * B / HBM_BPS, flops * B / MFMA_FLOPS
        bound = max(t_hbm, t_mfma)
        res["bound"] = "hbm" if t_hbm >= t_mfma else "mfma"
        res["share_of_bound_batch64"] = round(bound / dt, 4)
        res["share_of_bound_batch64_device"] = round(bound / (sp["device_ms"] / 1e3), 4)
print(json.dumps(res))

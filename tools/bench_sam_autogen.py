#!/usr/bin/env python3
"""Automatic mask generation on one sam_encode: the whole Model.sam_generate_masks_device call against Model.sam_compute_batch_device on the same prompts,
in the same build, on a synthetic full-size MobileSAM file (TinyViT-5M encoder, 1024 x 1024 image, the 32 x 32 grid of vision.sam_point_grid = 1024 prompts,
3072 candidates). Prints a text record and, last, ONE JSON line. A measurement, not a gate.

  * per chunk size of --chunks (default 64 and 256): the generate call and the batch call alternate within a sample, `--warmup` rounds of both first; host
    clock around each, stream NULL, so both end synchronised; min / median / max over --samples. Both leave their outputs on the device. The batch call
    writes 1024 masks of 1 MB; the generate call keeps the 1024 x 4 logit planes (512 MB) and writes at most --max-masks masks.
  * three settings of the thresholds, because the synthetic weights predict no iou above SAM's 0.88 and their masks are noise whose boxes are the whole
    plane: "defaults" (SAM's: nothing survives the filters here, the selection stage has nothing to rank), "all-to-nms" (filters open, NMS at 0.7: all 3072
    candidates are ranked, one survives NMS) and "all-kept" (filters open, NMS at 1.0, which suppresses nobody: 3072 kept, --max-masks come out).
  * the split decode / scoring / rank + NMS / output masks of the generate call by HIP events (Model.enable_timing; a run of its own, since the events make
    the call wait): medians over --samples.
  * vx_sam_rank_nms alone at N = 16384 candidates by HIP events: all boxes disjoint (every row of the suppression matrix is read by the scan), all boxes
    identical (one survivor) and a quarter of the candidates surviving the filters.

    python tools/bench_sam_autogen.py [--warmup 2] [--samples 7] [--chunks 64,256] [--max-masks 256]"""
import argparse
import ctypes
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
from visioncpp_amd import synth, vision  # noqa: E402

SETTINGS = {"defaults": dict(), "all-to-nms": dict(pred_iou_thresh=-1e30, stability_thresh=-1.0, nms_iou_thresh=0.7),
            "all-kept": dict(pred_iou_thresh=-1e30, stability_thresh=-1.0, nms_iou_thresh=1.0)}


def stats(ts, digits=1):
    return dict(min=round(float(min(ts)), digits), median=round(float(np.median(ts)), digits), max=round(float(max(ts)), digits))


def events_ms(fn, samples, warmup):
    """median / min / max ms of fn() between two HIP events on the null stream"""
    api = U.api()
    e0, e1 = ctypes.c_void_p(), ctypes.c_void_p()
    L.vx_check(api.vx_event_create(ctypes.byref(e0)))
    L.vx_check(api.vx_event_create(ctypes.byref(e1)))
    ts = []
    for i in range(warmup + samples):
        L.vx_check(api.vx_event_record(e0, None))
        fn()
        L.vx_check(api.vx_event_record(e1, None))
        ms = ctypes.c_float()
        L.vx_check(api.vx_event_elapsed_ms(e0, e1, ctypes.byref(ms)))
        if i >= warmup:
            ts.append(ms.value)
    L.vx_check(api.vx_event_destroy(e0))
    L.vx_check(api.vx_event_destroy(e1))
    return stats(ts, 3)


def nms_alone(samples, warmup):
    api, N, cap = U.api(), 16384, 256
    i = np.arange(N)
    disjoint = np.stack([2 * (i % 128), 2 * (i // 128), 2 * (i % 128) + 1, 2 * (i // 128) + 1], 1)
    identical = np.tile([10, 20, 200, 220], (N, 1))
    rng = np.random.default_rng(0)
    x0, y0 = rng.integers(0, 200, N), rng.integers(0, 200, N)
    random_boxes = np.stack([x0, y0, x0 + rng.integers(1, 56, N), y0 + rng.integers(1, 56, N)], 1)
    iou = (0.5 + 0.5 * rng.random(N)).astype(np.float32)
    rows = {}
    ws_bytes = api.vx_sam_rank_nms_workspace_bytes(N)
    ws = U.empty(ws_bytes, zero=False)
    flags, rank, keep, counts = U.empty(N * 4), U.empty(N * 4), U.empty(cap * 4), U.empty(8)
    for name, boxes, pt in (("disjoint", disjoint, 0.0), ("identical", identical, 0.0), ("random, a quarter survive the filters", random_boxes, 0.875)):
        table = np.zeros((N, 6), np.int32)
        table[:, 0], table[:, 1], table[:, 2:] = 3, 4, boxes
        t, io = U.dev(table), U.dev(iou)

        def run():
            L.vx_check(api.vx_sam_rank_nms(t.ptr, io.ptr, 1, 1, N, pt, 0.5, 0.7, cap, ws.ptr, ws_bytes, flags.ptr, rank.ptr, keep.ptr, counts.ptr, None))

        ms = events_ms(run, samples, warmup)
        U.sync()
        c = counts.to_numpy(np.int32, (2,))
        rows[name] = dict(ms=ms, survivors=int(flags.to_numpy(np.int32, (N,)).sum()), kept=int(c[1]), returned=int(c[0]))
        print(f"vx_sam_rank_nms alone, N = {N}, {name}: {ms} ms; {rows[name]['survivors']} survive the filters, {c[1]} kept, {c[0]} returned")
    return dict(N=N, capacity=cap, workspace_bytes=int(ws_bytes), cases=rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--samples", type=int, default=7)
    ap.add_argument("--chunks", default="64,256")
    ap.add_argument("--max-masks", type=int, default=256)
    a = ap.parse_args()
    chunks = [int(c) for c in a.chunks.split(",")]
    assert U.api().vx_device_count() > 0, "no HIP device visible: there is nothing to measure without one"
    device = vision.Device.init(vision.Backend.gpu)
    prompts = [list(map(int, p)) for p in vision.sam_point_grid(32, 1024, 1024)]
    P, cap = len(prompts), a.max_masks
    rows = []
    with tempfile.TemporaryDirectory() as td:
        path = synth.write_mobile_sam_gguf(Path(td) / "mobile_sam.gguf", synth.TINYVIT_5M, seed=0)
        model = vision.Model.load(path, device)
        model.sam_encode(np.random.default_rng(2).integers(0, 256, (1024, 1024, 3), dtype=np.uint8))
        bm, bi, bc = U.empty(P * 1024 * 1024, zero=False), U.empty(P * 16, zero=False), U.empty(P * 4, zero=False)
        gm, gi, gf, gc = U.empty(cap * 1024 * 1024, zero=False), U.empty(cap * 32, zero=False), U.empty(cap * 8, zero=False), U.empty(8)
        print(f"MobileSAM automatic mask generation, {P} grid prompts ({3 * P} candidates) on one embedding, at most {cap} masks out; warm-up {a.warmup} rounds, "
              f"{a.samples} samples")

        def batch():
            t0 = time.perf_counter()
            model.sam_compute_batch_device(prompts, bm.ptr, bi.ptr, bc.ptr)
            return (time.perf_counter() - t0) * 1e3

        for chunk in chunks:
            model.sam_set_prompt_chunk(chunk)
            for name, kw in SETTINGS.items():
                def generate():
                    t0 = time.perf_counter()
                    model.sam_generate_masks_device(prompts, gm.ptr, gi.ptr, gf.ptr, gc.ptr, max_masks=cap, **kw)
                    return (time.perf_counter() - t0) * 1e3

                for _ in range(a.warmup):
                    generate()
                    batch()
                tg, tb = [], []
                for _ in range(a.samples):
                    tg.append(generate())
                    tb.append(batch())
                counts = gc.to_numpy(np.int32, (2,))
                model.enable_timing(True)
                splits = []
                for _ in range(a.samples):
                    generate()
                    splits.append(model.sam_generate_last_split())
                model.enable_timing(False)
                split = {k: round(float(np.median([s[k] for s in splits])), 3) for k in splits[0]}
                row = dict(chunk=chunk, thresholds=name, generate_ms=stats(tg, 2), batch_ms=stats(tb, 2),
                           generate_over_batch=round(float(np.median(tg)) / float(np.median(tb)), 3), returned=int(counts[0]), kept=int(counts[1]), split_ms=split)
                rows.append(row)
                print(f"chunk {chunk}, {name}: generate {row['generate_ms']} ms, batch {row['batch_ms']} ms, generate / batch {row['generate_over_batch']}; "
                      f"{counts[1]} kept, {counts[0]} returned; split by events {split}")
        del model
        U.release()
    nms = nms_alone(a.samples, a.warmup)
    U.release()
    print(json.dumps(dict(tool="bench_sam_autogen", image=[1024, 1024], prompts=P, candidates=3 * P, max_masks=cap, chunks=chunks, rows=rows, rank_nms_alone=nms)))


if __name__ == "__main__":
    main()

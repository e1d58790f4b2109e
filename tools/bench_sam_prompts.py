#!/usr/bin/env python3
"""Many prompts on one sam_encode: a loop of the single-prompt sam_compute against one sam_compute_batch_device call, on a synthetic full-size MobileSAM
file (TinyViT-5M encoder, 64 x 64 x 256 embedding, 1024 x 1024 image). Prints a text record and, last, ONE JSON line. A measurement, not a gate.

  * P = 1, 8, 64, 256 and 1024 point prompts: the 32 x 32 grid of vision.sam_point_grid, thinned evenly for the smaller P.
  * loop: P calls of Model.sam_compute (each: the batched decoder with one prompt -- prompt on the host, upload, about 85 launches -- one mask back, one synchronise).
    batch: one Model.sam_compute_batch_device call into device buffers (masks u8 [P, 1024, 1024], iou, chosen), stream NULL, so it ends in a synchronise.
    Host clock around each; both end synchronised. The loop side brings every mask back to the host (that is what sam_compute does), the batch side leaves its
    masks on the device (that is what the device entry is for): the comparison is of the two calls as their users make them, not of equal work.
    Loop and batch alternate within a sample; `--warmup` rounds of both come first for every P and chunk size.
  * min / median / max over the samples, per prompt too. Fewer samples at the large P, where one sample is a second of work: 20, 20, 20, 7 and 5.
  * the masks of both sides are compared at P = 8 on the way (pixels differing).
  * every chunk size of --chunks (default 64 and 256) where P exceeds the previous one.

    python tools/bench_sam_prompts.py [--warmup 2] [--chunks 64,256] [--sizes 1,8,64,256,1024]"""
import argparse
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
from visioncpp_amd import synth, vision  # noqa: E402

SAMPLES = {1: 20, 8: 20, 64: 20, 256: 7, 1024: 5}


def stats(ts):
    return dict(min=round(float(min(ts)), 1), median=round(float(np.median(ts)), 1), max=round(float(max(ts)), 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--chunks", default="64,256")
    ap.add_argument("--sizes", default="1,8,64,256,1024")
    a = ap.parse_args()
    chunks = [int(c) for c in a.chunks.split(",")]
    sizes = [int(s) for s in a.sizes.split(",")]
    assert U.api().vx_device_count() > 0, "no HIP device visible: there is nothing to measure without one"
    device = vision.Device.init(vision.Backend.gpu)
    grid = vision.sam_point_grid(32, 1024, 1024)
    rows = []
    with tempfile.TemporaryDirectory() as td:
        path = synth.write_mobile_sam_gguf(Path(td) / "mobile_sam.gguf", synth.TINYVIT_5M, seed=0)
        model = vision.Model.load(path, device)
        model.sam_encode(np.random.default_rng(2).integers(0, 256, (1024, 1024, 3), dtype=np.uint8))
        print(f"MobileSAM, many prompts on one embedding: loop of sam_compute against sam_compute_batch_device; warm-up {a.warmup} rounds")
        for P in sizes:
            prompts = [list(map(int, p)) for p in grid[np.linspace(0, len(grid) - 1, P).round().astype(int)]]
            masks, iou, chosen = U.empty(P * 1024 * 1024, zero=False), U.empty(P * 16, zero=False), U.empty(P * 4, zero=False)
            use = [c for i, c in enumerate(chunks) if i == 0 or P > chunks[i - 1]]
            n = SAMPLES.get(P, 5)

            def loop():
                t0 = time.perf_counter()
                out = [model.sam_compute(p) for p in prompts]
                return (time.perf_counter() - t0) * 1e6, out

            def batch(chunk):
                model.sam_set_prompt_chunk(chunk)
                t0 = time.perf_counter()
                model.sam_compute_batch_device(prompts, masks.ptr, iou.ptr, chosen.ptr)
                return (time.perf_counter() - t0) * 1e6

            for _ in range(a.warmup):
                loop()
                for c in use:
                    batch(c)
            tl, tb = [], {c: [] for c in use}
            for _ in range(n):
                tl.append(loop()[0])
                for c in use:
                    tb[c].append(batch(c))
            row = dict(P=P, samples=n, loop_us=stats(tl), loop_us_per_prompt=round(float(np.median(tl)) / P, 1), batch={})
            for c in use:
                med = float(np.median(tb[c]))
                row["batch"][f"chunk{c}"] = dict(us=stats(tb[c]), us_per_prompt=round(med / P, 1), loop_over_batch=round(float(np.median(tl)) / med, 2))
            if P == 8:
                model.sam_set_prompt_chunk(use[0])
                model.sam_compute_batch_device(prompts, masks.ptr, iou.ptr, chosen.ptr)
                got = masks.to_numpy(np.uint8, (P, 1024, 1024))
                row["mask_pixels_differing_from_the_loop"] = float((got != np.stack(loop()[1])).mean())
            print(f"P = {P}: loop {row['loop_us']} us; " + "; ".join(f"{k}: batch {v['us']} us, {v['us_per_prompt']} us per prompt, loop / batch {v['loop_over_batch']}" for k, v in row["batch"].items())
                  + (f"; masks differ from the loop's on {row['mask_pixels_differing_from_the_loop']:.2e} of the pixels" if P == 8 else ""))
            rows.append(row)
            del masks, iou, chosen
            U.release()
        del model
    print(json.dumps(dict(tool="bench_sam_prompts", image=[1024, 1024], chunks=chunks, rows=rows)))


if __name__ == "__main__":
    main()

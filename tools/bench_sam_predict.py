#!/usr/bin/env python3
"""Model.sam_predict and the mask-input kernel behind it, on a synthetic full-size MobileSAM file (TinyViT-5M, 64 x 64 x 256 embedding, 1024 x 1024 image)
with the mask_downscaling tensors. Writes a text record (--out, default profiles/sam_predict_bench.txt) and prints, last, ONE JSON line. A measurement, not a gate.

  * vx_sam_dense_prompt_f16 at n = 1, 16, 64 (res 64, dim 256, f32 embedding, with pe): `--reps` launches back to back on the device's stream between two
    synchronisations, host clock, per launch; next to the time a device-to-device copy of as many bytes as the kernel reads and writes takes, measured the same way
    (mask 256 KB per prompt in; K and k1 2 MB each per prompt out; embedding and pe 4 + 2 MB once).
  * one refine round from the host: sam_predict with two points and the previous low-resolution logits, against sam_compute with one point.
  * 64 prompts with mask inputs (sam_predict_device, mask inputs and outputs on the device) against sam_compute_batch_device of 64 points.
  Every figure: median (min .. max) over --samples, after --warmup rounds.

    python tools/bench_sam_predict.py [--warmup 3] [--samples 20] [--reps 50] [--out FILE]"""
import argparse
import json
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
from __graft_entry__ import load_package  # noqa: E402

load_package()
from tests import gpu_util as U  # noqa: E402
from tests import sam_dense_ref as R  # noqa: E402
from visioncpp_amd import _lib as L, synth, vision  # noqa: E402


def timed(fn, warmup, samples):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(samples):
        U.sync()
        t0 = time.perf_counter()
        fn()
        U.sync()
        ts.append((time.perf_counter() - t0) * 1e6)
    return dict(median=round(float(np.median(ts)), 1), min=round(float(min(ts)), 1), max=round(float(max(ts)), 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--samples", type=int, default=20)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "sam_predict_bench.txt"))
    a = ap.parse_args()
    api = U.api()
    assert api.vx_device_count() > 0, "no HIP device visible: there is nothing to measure without one"
    device = vision.Device.init(vision.Backend.gpu)
    lines, result = [], dict(tool="bench_sam_predict", kernel=[], refine={}, batch64={})
    rng = np.random.default_rng(0)
    res, dim, S = 64, 256, 256
    W = R.weights(synth.sam_decoder_state_dict(1, mask_input=True))
    f32 = lambda x: U.dev(np.ascontiguousarray(x, np.float32)).ptr
    w = [f32(W[k]) for k in ("0.weight", "0.bias", "1.weight", "1.bias", "3.weight", "3.bias", "4.weight", "4.bias", "6.bias")]
    w3 = U.dev(W["6.weight"].reshape(dim, 16).astype(np.float16)).ptr
    embed, pe = f32(rng.standard_normal((res * res, dim))), U.dev(rng.standard_normal((res * res, dim)).astype(np.float16)).ptr
    for n in (1, 16, 64):
        mask = U.dev((5 * rng.standard_normal((n, S, S))).astype(np.float32))
        K, k1 = U.empty(n * res * res * dim * 2, zero=False), U.empty(n * res * res * dim * 2, zero=False)
        nbytes = n * S * S * 4 + 2 * n * res * res * dim * 2 + res * res * dim * 6
        src, dst = U.empty(nbytes // 2, zero=False), U.empty(nbytes // 2, zero=False)

        def kernel():
            for _ in range(a.reps):
                L.vx_check(api.vx_sam_dense_prompt_f16(mask.ptr, S * S, S, w[0], w[1], w[2], w[3], 4, w[4], w[5], w[6], w[7], 16, w3, w[8], embed, 1, pe, K.ptr, k1.ptr, n,
                                                       res, dim, R.EPS, None))

        def copy():
            for _ in range(a.reps):
                L.vx_check(api.vx_memcpy_d2d(dst.ptr, src.ptr, nbytes // 2, None))

        tk, tc = timed(kernel, a.warmup, a.samples), timed(copy, a.warmup, a.samples)
        row = dict(n=n, bytes=nbytes, kernel_us={k: round(v / a.reps, 2) for k, v in tk.items()}, copy_us={k: round(v / a.reps, 2) for k, v in tc.items()})
        row["kernel_over_copy"] = round(row["kernel_us"]["median"] / row["copy_us"]["median"], 2)
        row["GBps"] = round(nbytes / row["kernel_us"]["median"] / 1e3, 1)
        result["kernel"].append(row)
        lines.append(f"vx_sam_dense_prompt_f16 n = {n}: {row['kernel_us']} us per launch, {nbytes} bytes in + out = {row['GBps']} GB/s; a device copy moving as many bytes "
                     f"(half read, half written): {row['copy_us']} us; kernel / copy {row['kernel_over_copy']}")
    with tempfile.TemporaryDirectory() as td:
        path = synth.write_mobile_sam_gguf(Path(td) / "mobile_sam.gguf", synth.TINYVIT_5M, seed=0, dec_sd=synth.sam_decoder_state_dict(1000, mask_input=True))
        model = vision.Model.load(path, device)
        model.sam_encode(rng.integers(0, 256, (1024, 1024, 3), dtype=np.uint8))
        pts, lab = [[700, 300], [300, 800]], [1, 0]
        low = model.sam_predict(pts, lab)[3]
        result["refine"] = dict(sam_compute_one_point_us=timed(lambda: model.sam_compute([700, 300]), a.warmup, a.samples),
                                sam_predict_one_point_us=timed(lambda: model.sam_predict([[700, 300]]), a.warmup, a.samples),
                                sam_predict_two_points_mask_us=timed(lambda: model.sam_predict(pts, lab, mask_input=low), a.warmup, a.samples))
        lines.append(f"one prompt from the host (1024 x 1024 mask back): {result['refine']}")
        P = 64
        grid = vision.sam_point_grid(8, 1024, 1024)
        bp = np.stack([grid, grid[::-1]], axis=1).astype(np.int32)  # [64, 2, 2]
        bl = np.tile(np.array([1, 0], np.int32), (P, 1))
        masks, iou, chosen, lows = U.empty(P * 1024 * 1024, zero=False), U.empty(P * 16, zero=False), U.empty(P * 4, zero=False), U.empty(P * S * S * 4, zero=False)
        model.sam_predict_device(bp, bl, masks_dev=masks.ptr, iou_dev=iou.ptr, chosen_dev=chosen.ptr, low_res_dev=lows.ptr)
        prompts = [list(map(int, p)) for p in grid]
        result["batch64"] = dict(
            sam_compute_batch_device_points_us=timed(lambda: model.sam_compute_batch_device(prompts, masks.ptr, iou.ptr, chosen.ptr), a.warmup, a.samples),
            sam_predict_device_two_points_us=timed(lambda: model.sam_predict_device(bp, bl, masks_dev=masks.ptr, iou_dev=iou.ptr, chosen_dev=chosen.ptr), a.warmup, a.samples),
            sam_predict_device_two_points_mask_us=timed(lambda: model.sam_predict_device(bp, bl, mask_input_dev=lows.ptr, masks_dev=masks.ptr, iou_dev=iou.ptr, chosen_dev=chosen.ptr),
                                                        a.warmup, a.samples))
        lines.append(f"64 prompts, outputs on the device: {result['batch64']}")
        del model
        U.release()
    head = f"tools/bench_sam_predict.py on one MI355X (gfx950): warm-up {a.warmup}, {a.samples} samples, {a.reps} launches per kernel sample; us, median (min, max)"
    Path(a.out).write_text("\n".join([head] + lines) + "\n")
    print("\n".join([head] + lines))
    print(json.dumps(result))


if __name__ == "__main__":
    main()

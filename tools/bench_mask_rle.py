#!/usr/bin/env python3
"""Run-length encoding of masks on the device (vx_mask_rle_u8) and the generate call with RLE records, in the style of tools/bench_sam_regions.py and on its
scenario: the synthetic full-size MobileSAM file, a 1024 x 1024 image, the 32 x 32 grid, "all kept", at most --max-masks masks out. Prints a text record
and, last, ONE JSON line. A measurement, not a gate.

  1. the kernel alone by HIP events around the launcher (stream NULL, buffers allocated once): the generated masks (blobs), the same masks one byte off
     alignment (the kernel's byte path) and as many masks of density-0.5 noise (run-heavy), the full form and the count-only form, next to the time to read the masks once at bench.py's HBM rate -- the floor of a kernel that
     reads each mask once.
  2. the call: visp_sam_generate_masks_rle_host against visp_sam_generate_masks_host (what the Python layer calls at min_mask_region_area 0) on the same prompts and thresholds, alternating within a sample,
     host clock around the blocking calls; the bytes each moves to the host, summed from the copies the entries issue (binary: counts [2], the returned
     masks and records; RLE: counts [2], n_runs [max_masks], exactly the runs, the records -- and max_masks + 1 offsets UP to the device); and, for scale, the host-side encode of the same masks (tests/rle_ref.py's
     definition, vectorised with numpy).

    python tools/bench_mask_rle.py [--warmup 2] [--samples 7] [--max-masks 256] [--host-masks 16]"""
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
from tests import sam_select_ref as R  # noqa: E402
from tools.bench_sam_regions import events_ms, stats  # noqa: E402
from visioncpp_amd import _lib as L  # noqa: E402
from visioncpp_amd import synth, vision  # noqa: E402

PEAK_HBM = 8.0e12  # bench.py's
ALL_KEPT = dict(pred_iou_thresh=-1e30, stability_thresh=-1.0, nms_iou_thresh=1.0)


def numpy_rle(mask):
    """the reference's definition without its loop: what SAM's mask_to_rle_pytorch does on the host"""
    bits = np.asarray(mask != 0).T.ravel()
    b = np.flatnonzero(np.diff(bits, prepend=False))
    return np.diff(np.concatenate([[0], b, [bits.size]])).tolist()


def kernel_alone(name, masks_dev, n, w, h, samples, warmup):
    api = U.api()
    group = min(n, 256)
    ws_bytes = api.vx_mask_rle_workspace_bytes(w, h, group)
    ws, nr = U.empty(ws_bytes, zero=False), U.empty(n * 4)
    L.vx_check(api.vx_mask_rle_u8(masks_dev, w, h, n, None, None, 0, nr.ptr, ws.ptr, ws_bytes, group, None))
    U.sync()
    n_runs = nr.to_numpy(np.int32, (n,))
    stride = int(n_runs.max())
    rows = U.empty(n * stride * 4, zero=False)
    count = events_ms(lambda: L.vx_check(api.vx_mask_rle_u8(masks_dev, w, h, n, None, None, 0, nr.ptr, ws.ptr, ws_bytes, group, None)), samples, warmup)
    full = events_ms(lambda: L.vx_check(api.vx_mask_rle_u8(masks_dev, w, h, n, None, rows.ptr, stride, nr.ptr, ws.ptr, ws_bytes, group, None)), samples, warmup)
    floor_ms = n * w * h / PEAK_HBM * 1e3
    row = dict(masks=n, runs_total=int(n_runs.sum()), runs_max=stride, count_only_ms=count, full_ms=full, read_once_floor_ms=round(floor_ms, 4),
               count_only_over_floor=round(count["median"] / floor_ms, 2), full_over_floor=round(full["median"] / floor_ms, 2),
               run_bytes_written=int(n_runs.sum()) * 4)
    print(f"kernel alone, {name}: {row}")
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--samples", type=int, default=7)
    ap.add_argument("--max-masks", type=int, default=256)
    ap.add_argument("--host-masks", type=int, default=16, help="masks the numpy encode runs on (its time is scaled to the masks returned)")
    a = ap.parse_args()
    assert U.api().vx_device_count() > 0, "no HIP device visible: there is nothing to measure without one"
    device = vision.Device.init(vision.Backend.gpu)
    prompts = [list(map(int, p)) for p in vision.sam_point_grid(32, 1024, 1024)]
    cap, w, h = a.max_masks, 1024, 1024
    with tempfile.TemporaryDirectory() as td:
        cfg = synth.TINYVIT_5M
        path = synth.write_mobile_sam_gguf(Path(td) / "mobile_sam.gguf", cfg, enc_sd=synth.tinyvit_state_dict(cfg, 0), dec_sd=R.scenario_decoder_state_dict())
        model = vision.Model.load(path, device)
        model.sam_encode(np.random.default_rng(2).integers(0, 256, (h, w, 3), dtype=np.uint8))
        model.sam_set_prompt_chunk(256)
        gm, gi, gf, gc = U.empty(cap * w * h, zero=False), U.empty(cap * 32, zero=False), U.empty(cap * 8, zero=False), U.empty(16)
        model.sam_generate_masks_device(prompts, gm.ptr, gi.ptr, gf.ptr, gc.ptr, max_masks=cap, **ALL_KEPT)
        U.sync()
        k = int(gc.to_numpy(np.int32, (2,))[0])
        kernel = {"generated": kernel_alone("generated masks", gm.ptr, k, w, h, a.samples, a.warmup)}
        noise = np.where(np.random.default_rng(0).random((8, h, w)) < 0.5, 255, 0).astype(np.uint8)
        # the byte path: the same masks one byte off a 16-byte boundary (what any width that is no multiple of 16 takes as well)
        off = U.empty(k * w * h + 16, zero=False)
        L.vx_check(U.api().vx_memcpy_d2d(off.ptr + 1, gm.ptr, k * w * h, None))
        U.sync()
        kernel["generated_byte_path"] = kernel_alone("generated masks, base + 1: the byte path", off.ptr + 1, k, w, h, a.samples, a.warmup)
        nd = U.dev(np.concatenate([noise] * (k // 8)) if k >= 8 else noise[:k])
        kernel["noise_0.5"] = kernel_alone("density-0.5 noise", nd.ptr, k if k < 8 else k // 8 * 8, w, h, a.samples, a.warmup)

        def binary():
            t0 = time.perf_counter()
            out = model.sam_generate_masks_raw(prompts, max_masks=cap, **ALL_KEPT)
            return (time.perf_counter() - t0) * 1e3, out

        def rle():
            t0 = time.perf_counter()
            out = model.sam_generate_masks_rle_raw(prompts, max_masks=cap, **ALL_KEPT)
            return (time.perf_counter() - t0) * 1e3, out

        for _ in range(a.warmup):
            binary(), rle()
        t_bin, t_rle = [], []
        for _ in range(a.samples):
            tb, (masks, ii, _, _) = binary()
            tr, (recs, _, _, _) = rle()
            t_bin.append(tb)
            t_rle.append(tr)
        n_host = min(a.host_masks, len(masks))
        t0 = time.perf_counter()
        host = [numpy_rle(m) for m in masks[:n_host]]
        host_ms = (time.perf_counter() - t0) * 1e3
        assert host == [r["counts"] for r in recs[:n_host]], "the device's runs differ from the host encode of the binary entry's masks"
        runs = sum(len(r["counts"]) for r in recs)
        call = dict(returned=len(recs), binary_entry_ms=stats(t_bin), rle_entry_ms=stats(t_rle), median_difference_ms=round(float(np.median(t_bin) - np.median(t_rle)), 2),
                    binary_bytes_to_host=int(8 + masks.nbytes + len(masks) * (32 + 8)), rle_bytes_to_host=int(8 + cap * 4 + runs * 4 + len(recs) * (32 + 8)), rle_bytes_to_device=int((len(recs) + 1) * 8),
                    numpy_encode=dict(masks=n_host, ms=round(host_ms, 1), scaled_to_returned_ms=round(host_ms / max(n_host, 1) * len(recs), 1)))
        print(f"the call, {len(prompts)} prompts, all kept, {len(recs)} masks out (both entries through the Python layer, which also builds the RLE dicts): {call}")
        del model
        U.release()
    print(json.dumps(dict(tool="bench_mask_rle", image=[w, h], prompts=len(prompts), max_masks=cap, kernel_alone=kernel, call=call)))


if __name__ == "__main__":
    main()

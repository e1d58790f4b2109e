#!/usr/bin/env python3
"""COCO's compressed counts strings on the device (kernels_rle_codec.hip), on the scenario of tools/bench_mask_rle.py and tools/bench_mask_rle_decode.py: the
synthetic full-size MobileSAM file, a 1024 x 1024 image, the 32 x 32 grid, "all kept", at most --max-masks masks. Prints a text record and writes ONE JSON
line to --out. A measurement, not a gate.

  1. the launchers alone by HIP events (stream NULL, buffers allocated once) on the records of the generated masks: vx_rle_compress count pass, its write call
     (which runs the count again: three launches) and vx_rle_decompress count pass and write pass.
  2. one long record (--long-runs runs, the checkerboard of a 316 x 316 mask is that long) through the same four, for the split of a record over blocks.
  3. masks -> strings end to end by the host clock around vision.mask_to_coco_rle, next to vision.mask_to_rle on the same masks, and the bytes each reads
     back: the strings against the uncompressed runs.

    python tools/bench_mask_rle_codec.py [--warmup 2] [--samples 7] [--max-masks 256] [--long-runs 100000] [--out profiles/mask_rle_codec_bench.txt]"""
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
from tests import rle_codec_ref as ref  # noqa: E402
from tests import sam_select_ref as R  # noqa: E402
from tools.bench_mask_rle import ALL_KEPT  # noqa: E402
from tools.bench_sam_regions import events_ms, stats  # noqa: E402
from visioncpp_amd import _lib as L  # noqa: E402
from visioncpp_amd import synth, vision  # noqa: E402


def launchers(api, rows, samples, warmup):
    """rows of counts -> the four passes by HIP events, checked against the reference on the first and the last record"""
    n = len(rows)
    offsets, runs = vision._run_rows([{"counts": r} for r in rows])
    total, longest = int(offsets[-1]), max(len(r) for r in rows)
    rd, od, sd = U.dev(runs), U.dev(offsets), U.empty(n * 4)
    ws = api.vx_rle_compress_workspace_bytes(total, n)
    wd = U.empty(ws)

    def count():
        L.vx_check(api.vx_rle_compress(rd.ptr, od.ptr, total, longest, n, None, 0, None, None, sd.ptr, wd.ptr, ws, None))

    count()
    boff = np.concatenate([[0], np.cumsum(sd.to_numpy(np.int32, (n,)))]).astype(np.int64)
    bd, bod = U.empty(int(boff[-1]) + 16, zero=False), U.dev(boff)

    def write():
        L.vx_check(api.vx_rle_compress(rd.ptr, od.ptr, total, longest, n, None, 0, bd.ptr, bod.ptr, None, wd.ptr, ws, None))

    out, rod, nd = U.empty(total * 4 + 16, zero=False), U.dev(offsets), U.empty(n * 4)

    def back_count():
        L.vx_check(api.vx_rle_decompress(bd.ptr, bod.ptr, n, None, 0, None, None, nd.ptr, None, None))

    def back_write():
        L.vx_check(api.vx_rle_decompress(bd.ptr, bod.ptr, n, None, 0, out.ptr, rod.ptr, None, None, None))

    res = dict(records=n, runs_total=total, longest_record=longest, string_bytes=int(boff[-1]), compress_count_ms=events_ms(count, samples, warmup),
               compress_write_ms=events_ms(write, samples, warmup), decompress_count_ms=events_ms(back_count, samples, warmup),
               decompress_write_ms=events_ms(back_write, samples, warmup))
    strings = bd.to_numpy(np.uint8, (int(boff[-1]),)).tobytes()
    for b in (0, n - 1):
        assert strings[int(boff[b]):int(boff[b + 1])] == ref.enc(rows[b]), f"record {b}: the device's string differs from the reference's"
    assert np.array_equal(out.to_numpy(np.uint32, (total,)), runs[:total]) and np.array_equal(nd.to_numpy(np.int32, (n,)), np.diff(offsets)), "the way back differs"
    res["bytes_per_run"] = round(res["string_bytes"] / max(total, 1), 3)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--samples", type=int, default=7)
    ap.add_argument("--max-masks", type=int, default=256)
    ap.add_argument("--long-runs", type=int, default=100000)
    ap.add_argument("--out", default=str(Path(__file__).resolve().parents[1] / "profiles" / "mask_rle_codec_bench.txt"))
    a = ap.parse_args()
    api = U.api()
    assert api.vx_device_count() > 0, "no HIP device visible: there is nothing to measure without one"
    device = vision.Device.init(vision.Backend.gpu)
    prompts = [list(map(int, p)) for p in vision.sam_point_grid(32, 1024, 1024)]
    w, h = 1024, 1024
    with tempfile.TemporaryDirectory() as td:
        cfg = synth.TINYVIT_5M
        path = synth.write_mobile_sam_gguf(Path(td) / "mobile_sam.gguf", cfg, enc_sd=synth.tinyvit_state_dict(cfg, 0), dec_sd=R.scenario_decoder_state_dict())
        model = vision.Model.load(path, device)
        model.sam_encode(np.random.default_rng(2).integers(0, 256, (h, w, 3), dtype=np.uint8))
        model.sam_set_prompt_chunk(256)
        masks = model.sam_generate_masks_raw(prompts, max_masks=a.max_masks, **ALL_KEPT)[0]
        del model
    records = vision.mask_to_rle(masks, device=device)
    generated = launchers(api, [r["counts"] for r in records], a.samples, a.warmup)
    print(f"launchers alone, the generated masks' records: {generated}")
    one_long = launchers(api, [[1 + (i * 7919) % 3000 for i in range(a.long_runs)]], a.samples, a.warmup)
    print(f"launchers alone, one long record: {one_long}")

    t_packed, t_plain = [], []
    for i in range(a.warmup + a.samples):
        t0 = time.perf_counter()
        packed = vision.mask_to_coco_rle(masks, device=device)
        t1 = time.perf_counter()
        plain = vision.mask_to_rle(masks, device=device)
        t2 = time.perf_counter()
        if i >= a.warmup:
            t_packed.append((t1 - t0) * 1e3)
            t_plain.append((t2 - t1) * 1e3)
    assert all(p["counts"] == ref.enc(q["counts"]) for p, q in zip(packed[:4], plain[:4])), "the chained call's strings differ from the reference's"
    n = len(masks)
    end_to_end = dict(masks=n, mask_to_coco_rle_ms=stats(t_packed), mask_to_rle_ms=stats(t_plain), read_back_bytes=dict(strings=sum(len(p["counts"]) for p in packed) + 8 * n,
                      runs=4 * sum(len(q["counts"]) for q in plain) + 4 * n), upload_bytes=int(masks.size))
    print(f"masks -> strings end to end (both include the upload of the masks): {end_to_end}")
    U.release()
    line = json.dumps(dict(tool="bench_mask_rle_codec", image=[w, h], prompts=len(prompts), max_masks=a.max_masks, generated=generated, one_long=one_long, end_to_end=end_to_end))
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(line + "\n")
    print(line)


if __name__ == "__main__":
    main()

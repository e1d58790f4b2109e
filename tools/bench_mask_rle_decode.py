#!/usr/bin/env python3
"""RLE records back to masks on the device and the pairwise IoU of masks (kernels_rle_decode.hip), on the scenario of tools/bench_mask_rle.py: the synthetic
full-size MobileSAM file, a 1024 x 1024 image, the 32 x 32 grid, "all kept", at most --max-masks masks out as RLE records. Prints a text record and writes
ONE JSON line to --out. A measurement, not a gate.

  1. decode by HIP events around the two launchers (stream NULL, buffers allocated once): vx_rle_to_bits, vx_bits_to_mask_u8 and both, next to the time to
     write n h w bytes once at bench.py's HBM rate -- the floor of a kernel that writes each mask once.
  2. the host entry (vision.rle_decode: records up, decode, masks down) by the host clock around the blocking call, next to vision.rle_to_mask, the host loop,
     on --host-masks of the same records (scaled to all of them).
  3. the IoU matrix of the masks against themselves by HIP events around vx_bitmask_iou on their bit words, next to the AND + popcount word pairs it forms.

    python tools/bench_mask_rle_decode.py [--warmup 2] [--samples 7] [--max-masks 256] [--host-masks 8] [--out profiles/mask_rle_decode_bench.txt]"""
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
from tools.bench_mask_rle import ALL_KEPT, PEAK_HBM  # noqa: E402
from tools.bench_sam_regions import events_ms, stats  # noqa: E402
from visioncpp_amd import _lib as L  # noqa: E402
from visioncpp_amd import synth, vision  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--samples", type=int, default=7)
    ap.add_argument("--max-masks", type=int, default=256)
    ap.add_argument("--host-masks", type=int, default=8, help="records vision.rle_to_mask runs on (its time is scaled to the records returned)")
    ap.add_argument("--out", default=str(Path(__file__).resolve().parents[1] / "profiles" / "mask_rle_decode_bench.txt"))
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
        records = model.sam_generate_masks_rle_raw(prompts, max_masks=a.max_masks, **ALL_KEPT)[0]
        del model
    n = len(records)
    offsets, runs, _, _ = vision._rle_rows(records)
    rd, od = U.dev(runs), U.dev(offsets)
    per_mask = api.vx_mask_rle_workspace_bytes(w, h, 1)
    words, masks = U.empty(n * per_mask, zero=False), U.empty(n * w * h, zero=False)
    pos_bytes = api.vx_rle_to_bits_workspace_bytes(len(runs), n)
    pos = U.empty(pos_bytes, zero=False)

    def to_bits():
        L.vx_check(api.vx_rle_to_bits(rd.ptr, od.ptr, len(runs), n, w, h, None, 0, words.ptr, None, None, pos.ptr, pos_bytes, None))

    def to_masks():
        L.vx_check(api.vx_bits_to_mask_u8(words.ptr, n, w, h, None, 0, 255, masks.ptr, None))

    floor_ms = n * w * h / PEAK_HBM * 1e3
    both = events_ms(lambda: (to_bits(), to_masks()), a.samples, a.warmup)
    decode = dict(masks=n, runs_total=int(offsets[-1]), runs_to_bits_ms=events_ms(to_bits, a.samples, a.warmup), bits_to_masks_ms=events_ms(to_masks, a.samples, a.warmup),
                  both_ms=both, write_once_floor_ms=round(floor_ms, 4), both_over_floor=round(both["median"] / floor_ms, 2))
    print(f"decode, launchers alone: {decode}")

    t_entry = []
    for i in range(a.warmup + a.samples):
        t0 = time.perf_counter()
        got = vision.rle_decode(records, value=1, device=device)
        if i >= a.warmup:
            t_entry.append((time.perf_counter() - t0) * 1e3)
    n_host = min(a.host_masks, n)
    t0 = time.perf_counter()
    host = [vision.rle_to_mask(r) for r in records[:n_host]]
    host_ms = (time.perf_counter() - t0) * 1e3
    assert all(np.array_equal(m, g != 0) for m, g in zip(host, got)), "the device's masks differ from vision.rle_to_mask's"
    entry = dict(records=n, rle_decode_ms=stats(t_entry), rle_to_mask=dict(records=n_host, ms=round(host_ms, 1), scaled_to_all_ms=round(host_ms / max(n_host, 1) * n, 1)))
    print(f"the host entry against the host loop: {entry}")

    ws = api.vx_bitmask_iou_workspace_bytes(n, n)
    areas, out_iou, out_inter = U.empty(ws, zero=False), U.empty(n * n * 4, zero=False), U.empty(n * n * 4, zero=False)
    t_iou = events_ms(lambda: L.vx_check(api.vx_bitmask_iou(words.ptr, n, words.ptr, n, w, h, None, None, None, out_inter.ptr, out_iou.ptr, areas.ptr, ws, None)),
                      a.samples, a.warmup)
    inter = out_inter.to_numpy(np.int32, (n, n))
    assert np.array_equal(np.diag(inter), vision.rle_area(records)), "a mask's intersection with itself is not its area"
    word_pairs = n * n * w * (h // 64)
    iou = dict(matrix=[n, n], ms=t_iou, word_pairs=word_pairs, word_pairs_per_ns=round(word_pairs / (t_iou["median"] * 1e6), 1),
               bit_words_bytes_per_side=n * per_mask)
    print(f"the IoU matrix on bit words: {iou}")
    U.release()
    line = json.dumps(dict(tool="bench_mask_rle_decode", image=[w, h], prompts=len(prompts), max_masks=a.max_masks, decode=decode, host_entry=entry, iou=iou))
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(line + "\n")
    print(line)


if __name__ == "__main__":
    main()

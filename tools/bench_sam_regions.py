#!/usr/bin/env python3
"""The region-cleaning stage of automatic mask generation (min_mask_region_area) on one sam_encode, in the style of tools/bench_sam_autogen.py: a synthetic
full-size MobileSAM file whose decoder keeps the hypernetwork bias shift of tests/sam_select_ref.scenario_decoder_state_dict (so the masks are not pure noise),
a 1024 x 1024 image, the 32 x 32 grid = 1024 prompts, at most --max-masks masks out, the settings "all-to-nms" and "all-kept" of that tool. Prints a text
record and, last, ONE JSON line. A measurement, not a gate.

  * min_region_area 0 must cost nothing: visp_sam_generate_masks_clean_device(.., 0, ..) and visp_sam_generate_masks_device alternate within a sample, host
    clock, stream NULL; min / median / max over --samples. (The parent commit's own figures come from running this tool with --existing-only on a build of
    the parent: the bar is the parent's median plus its max - min.)
  * the cleaning stage by HIP events at min_region_area 100 and 1000 (Model.enable_timing; a run of its own): decode, scoring, rank + NMS, output masks, and
    the stage as clean / records + second NMS / gather; and what the call returned.
  * the primitive alone, vision.remove_small_regions_device on --max-masks masks of 1024^2 at three densities of random foreground, by HIP events around the
    launcher (the entry itself allocates and synchronises per call: its host time is printed next to it).
  * the bytes the stage moves per mask, counted from the layout, against the time: how far from the HBM rate.
  * the host baseline a caller would otherwise run: scipy.ndimage.label on the same masks (SAM's remove_small_regions, transcribed), one process.

    python tools/bench_sam_regions.py [--warmup 2] [--samples 7] [--chunks 64,256] [--max-masks 256] [--existing-only] [--host-masks 16]"""
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
from tests import sam_select_ref as R  # noqa: E402
from visioncpp_amd import _lib as L  # noqa: E402
from visioncpp_amd import synth, vision  # noqa: E402

SETTINGS = {"all-to-nms": dict(pred_iou_thresh=-1e30, stability_thresh=-1.0, nms_iou_thresh=0.7),
            "all-kept": dict(pred_iou_thresh=-1e30, stability_thresh=-1.0, nms_iou_thresh=1.0)}
HBM_GBS = 8000.0  # the MI355X's nominal HBM3E rate, for the distance only


def stats(ts, digits=2):
    return dict(min=round(float(min(ts)), digits), median=round(float(np.median(ts)), digits), max=round(float(max(ts)), digits),
                spread=round(float(max(ts) - min(ts)), digits))


def events_ms(fn, samples, warmup):
    api = U.api()
    e0, e1 = ctypes.c_void_p(), ctypes.c_void_p()
    L.vx_check(api.vx_event_create(ctypes.byref(e0)))
    L.vx_check(api.vx_event_create(ctypes.byref(e1)))
    ts = []
    for i in range(warmup + samples):
        L.vx_check(api.vx_event_record(e0, None))
        fn()
        L.vx_check(api.vx_event_record(e1, None))
        L.vx_check(api.vx_event_sync(e1))
        ms = ctypes.c_float()
        L.vx_check(api.vx_event_elapsed_ms(e0, e1, ctypes.byref(ms)))
        if i >= warmup:
            ts.append(ms.value)
    L.vx_check(api.vx_event_destroy(e0))
    L.vx_check(api.vx_event_destroy(e1))
    return stats(ts, 3)


def sam_remove_small_regions_scipy(mask, area_thresh, mode):
    """SAM's remove_small_regions with scipy's labelling in cv2's place: what a caller runs on the host today"""
    from scipy import ndimage
    correct_holes = mode == "holes"
    working = (correct_holes ^ mask).astype(np.uint8)
    regions, n = ndimage.label(working, structure=np.ones((3, 3), int))
    sizes = np.bincount(regions.reshape(-1), minlength=n + 1)[1:]
    small = [i + 1 for i, s in enumerate(sizes) if s < area_thresh]
    if not small:
        return mask, False
    fill = [0] + small
    if not correct_holes:
        fill = [i for i in range(n + 1) if i not in fill] or [int(np.argmax(sizes)) + 1]
    return np.isin(regions, fill), True


def bytes_per_mask(px, modes=2):
    """per step: tile reads the mask (1) and writes labels and areas (8); merge touches the tile borders only; areas reads labels and areas (8); best (islands)
    reads labels (4); decide reads labels (4), gathers areas at the roots and writes the flipped pixels. Two steps, the best pass once."""
    per_step = px * (1 + 8 + 8 + 4)
    return modes * per_step + px * 4


def primitive_alone(n, samples, warmup, min_area):
    api, w, h = U.api(), 1024, 1024
    rows = {}
    group = min(n, 32)
    ws_bytes = api.vx_mask_regions_workspace_bytes(w, h, group)
    ws, changed = U.empty(ws_bytes, zero=False), U.empty(n * 4)
    rng = np.random.default_rng(0)
    for density in (0.05, 0.5, 0.95):
        one = np.where(rng.random((8, h, w)) < density, 255, 0).astype(np.uint8)
        src = U.dev(np.concatenate([one] * (n // 8)) if n >= 8 else one[:n])
        work = U.empty(n * w * h, zero=False)

        def run():
            L.vx_check(api.vx_memcpy_d2d(work.ptr, src.ptr, n * w * h, None))
            L.vx_check(api.vx_mask_remove_small_regions_u8(work.ptr, w, h, n, None, min_area, 3, changed.ptr, ws.ptr, ws_bytes, group, None))

        def copy_only():
            L.vx_check(api.vx_memcpy_d2d(work.ptr, src.ptr, n * w * h, None))

        ms, copy = events_ms(run, samples, warmup), events_ms(copy_only, samples, warmup)
        U.sync()
        net = ms["median"] - copy["median"]
        t0 = time.perf_counter()
        vision.remove_small_regions_device(work.ptr, n, w, h, min_area, "both", changed.ptr)
        entry_ms = (time.perf_counter() - t0) * 1e3
        gb = n * bytes_per_mask(w * h) / 1e9
        rows[str(density)] = dict(ms=ms, copy_ms=copy, net_ms=round(net, 3), entry_host_ms=round(entry_ms, 2), counted_gb=round(gb, 2),
                                  gb_per_s=round(gb / (net * 1e-3), 1), of_hbm=round(gb / (net * 1e-3) / HBM_GBS, 3),
                                  changed=int(changed.to_numpy(np.int32, (n,)).sum()))
        print(f"primitive alone, {n} masks of 1024^2, density {density}, min_area {min_area}, groups of {group}: {ms} ms with the copy in ({copy} ms), net {net:.3f} ms; "
              f"{gb:.2f} GB counted = {rows[str(density)]['gb_per_s']} GB/s ({100 * rows[str(density)]['of_hbm']:.1f} % of {HBM_GBS:.0f}); the entry with its allocation: {entry_ms:.2f} ms host")
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--samples", type=int, default=7)
    ap.add_argument("--chunks", default="64,256")
    ap.add_argument("--max-masks", type=int, default=256)
    ap.add_argument("--areas", default="100,1000")
    ap.add_argument("--existing-only", action="store_true", help="only visp_sam_generate_masks_device: the figures of a build without the new entries")
    ap.add_argument("--host-masks", type=int, default=16, help="masks the scipy baseline runs on (its time is scaled to --max-masks)")
    a = ap.parse_args()
    chunks, areas = [int(c) for c in a.chunks.split(",")], [int(c) for c in a.areas.split(",")]
    assert U.api().vx_device_count() > 0, "no HIP device visible: there is nothing to measure without one"
    device = vision.Device.init(vision.Backend.gpu)
    prompts = [list(map(int, p)) for p in vision.sam_point_grid(32, 1024, 1024)]
    P, cap = len(prompts), a.max_masks
    rows, stage_rows, host = [], [], None
    with tempfile.TemporaryDirectory() as td:
        cfg = synth.TINYVIT_5M
        path = synth.write_mobile_sam_gguf(Path(td) / "mobile_sam.gguf", cfg, enc_sd=synth.tinyvit_state_dict(cfg, 0), dec_sd=R.scenario_decoder_state_dict())
        model = vision.Model.load(path, device)
        model.sam_encode(np.random.default_rng(2).integers(0, 256, (1024, 1024, 3), dtype=np.uint8))
        gm, gi, gf, gc = U.empty(cap * 1024 * 1024, zero=False), U.empty(cap * 32, zero=False), U.empty(cap * 8, zero=False), U.empty(16)
        print(f"MobileSAM region cleaning, {P} grid prompts ({3 * P} candidates) on one embedding, at most {cap} masks out; warm-up {a.warmup} rounds, {a.samples} samples")

        def call(area, kw, new_entry):
            t0 = time.perf_counter()
            if new_entry:
                p, k, params = model._sam_generate_args(prompts, 32, kw["pred_iou_thresh"], kw["stability_thresh"], None, kw["nms_iou_thresh"])
                L.check(model._api.visp_sam_generate_masks_clean_device(model._handle, p.ctypes.data, k.ctypes.data, len(k), *params, cap, area, gm.ptr, gi.ptr, gf.ptr,
                                                                        gc.ptr, None))
            else:
                model.sam_generate_masks_device(prompts, gm.ptr, gi.ptr, gf.ptr, gc.ptr, max_masks=cap, **kw)
            return (time.perf_counter() - t0) * 1e3

        for chunk in chunks:
            model.sam_set_prompt_chunk(chunk)
            for name, kw in SETTINGS.items():
                for _ in range(a.warmup):
                    call(0, kw, False)
                    a.existing_only or call(0, kw, True)
                t_old, t_new = [], []
                for _ in range(a.samples):
                    t_old.append(call(0, kw, False))
                    a.existing_only or t_new.append(call(0, kw, True))
                row = dict(chunk=chunk, thresholds=name, existing_ms=stats(t_old), clean_entry_area_0_ms=stats(t_new) if t_new else None)
                rows.append(row)
                print(f"chunk {chunk}, {name}: visp_sam_generate_masks_device {row['existing_ms']} ms; the new entry at min_region_area 0 {row['clean_entry_area_0_ms']} ms")
                if a.existing_only:
                    continue
                for area in areas:
                    for _ in range(a.warmup):
                        call(area, kw, True)
                    whole = [call(area, kw, True) for _ in range(a.samples)]
                    counts = gc.to_numpy(np.int32, (4,))
                    model.enable_timing(True)
                    splits = []
                    for _ in range(a.samples):
                        call(area, kw, True)
                        splits.append(model.sam_generate_last_split5())
                    model.enable_timing(False)
                    split = {k: round(float(np.median([s[k] for s in splits])), 3) for k in splits[0]}
                    spread = {k: round(float(max(s[k] for s in splits) - min(s[k] for s in splits)), 3) for k in ("clean_ms", "records_nms2_ms", "gather_ms")}
                    k_first = min(int(counts[1]), cap)
                    gb = k_first * bytes_per_mask(1024 * 1024) / 1e9
                    srow = dict(chunk=chunk, thresholds=name, min_region_area=area, generate_ms=stats(whole), split_ms=split, stage_spread_ms=spread, returned=int(counts[0]),
                                kept_first=int(counts[1]), changed=int(counts[2]), removed_second=int(counts[3]), cleaned_masks=k_first, counted_gb=round(gb, 2),
                                clean_gb_per_s=round(gb / (split["clean_ms"] * 1e-3), 1) if split["clean_ms"] > 0 else None)
                    stage_rows.append(srow)
                    print(f"chunk {chunk}, {name}, min_region_area {area}: generate {srow['generate_ms']} ms; by events {split} (max - min {spread}); {k_first} masks cleaned, "
                          f"{counts[2]} of the {counts[0]} returned changed, the second NMS removed {counts[3]}; {gb:.2f} GB counted in the clean = {srow['clean_gb_per_s']} GB/s")
        if not a.existing_only and a.host_masks > 0:
            model.sam_set_prompt_chunk(chunks[-1])
            kw = SETTINGS["all-kept"]
            call(0, kw, False)
            n_host = min(a.host_masks, int(gc.to_numpy(np.int32, (2,))[0]))
            masks = gm.to_numpy(np.uint8, (cap, 1024, 1024))[:n_host]
            host = {}
            for area in areas:
                t0 = time.perf_counter()
                for m in masks:
                    b, _ = sam_remove_small_regions_scipy(m != 0, area, "holes")
                    sam_remove_small_regions_scipy(b, area, "islands")
                dt = (time.perf_counter() - t0) * 1e3
                host[str(area)] = dict(masks=n_host, ms=round(dt, 1), ms_per_mask=round(dt / max(n_host, 1), 1), scaled_to_max_masks_ms=round(dt / max(n_host, 1) * cap, 0))
                print(f"host baseline (what a caller would otherwise run): scipy.ndimage.label, SAM's remove_small_regions on {n_host} of the generated masks, min_area {area}: "
                      f"{dt:.1f} ms = {dt / max(n_host, 1):.1f} ms per mask, {dt / max(n_host, 1) * cap / 1e3:.2f} s for {cap} (one process; plus the download)")
        del model
        U.release()
    alone = None if a.existing_only else primitive_alone(cap, a.samples, a.warmup, areas[0])
    U.release()
    print(json.dumps(dict(tool="bench_sam_regions", image=[1024, 1024], prompts=P, max_masks=cap, chunks=chunks, zero_cost=rows, stage=stage_rows, primitive_alone=alone,
                          host_baseline=host, bytes_per_mask_counted=bytes_per_mask(1024 * 1024))))


if __name__ == "__main__":
    main()

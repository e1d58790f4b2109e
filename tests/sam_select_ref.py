"""The selection stage of MobileSAM's automatic mask generation (csrc/kernels_samselect.hip, sam_generate_masks_device) restated in numpy: what the
device must compute, decision for decision. Every decision is an integer comparison or a float32 comparison of one float32 product, the forms the
kernels use, so equal inputs give equal decisions bit for bit. tests/test_sam_select_ref_cpu.py pins this file on independent code."""
from __future__ import annotations

import numpy as np

F = np.float32
DEFAULTS = dict(pred_iou_thresh=0.88, stability_thresh=0.95, stability_offset=1.0, nms_iou_thresh=0.7)
MAX_PROMPTS = 5461


def region(sw: int, sh: int, mask_size: int = 256, image_size: int = 1024):
    """(cw, ch): the part of a logit plane the image occupies, from the scaled extent sw x sh of sam_compute_batch_device"""
    return -(-sw * mask_size // image_size), -(-sh * mask_size // image_size)


def scaled_extent(w: int, h: int, image_size: int = 1024):
    """(sw, sh) as sam_compute_batch_device computes them, in float32"""
    up = F(image_size) / F(max(w, h))
    return int(F(w) * up + F(0.5)), int(F(h) * up + F(0.5))


def score_planes(planes, cw: int, ch: int, off):
    """planes [C, M, M] (float16 or float32 logits) -> (table int32 [C, 6] = {inter, uni, x0, y0, x1, y1}, stability float32 [C])"""
    planes = np.asarray(planes)
    r = planes[:, :ch, :cw].astype(F)
    off = F(off)
    C = r.shape[0]
    table = np.zeros((C, 6), np.int32)
    table[:, 0] = (r > off).reshape(C, -1).sum(1)
    table[:, 1] = (r > -off).reshape(C, -1).sum(1)
    for c in range(C):
        ys, xs = np.nonzero(r[c] > 0)
        if ys.size:
            table[c, 2:] = [xs.min(), ys.min(), xs.max(), ys.max()]
    inter, uni = table[:, 0].astype(F), table[:, 1].astype(F)
    with np.errstate(invalid="ignore", divide="ignore"):
        stability = np.where(table[:, 1] > 0, inter / uni, F(0)).astype(F)
    return table, stability


def filters(table, iou, pred_iou_thresh, stability_thresh):
    """-> bool [C]; iou float32 [C] per candidate"""
    iou = np.asarray(iou, F)
    with np.errstate(invalid="ignore"):
        return (iou > F(pred_iou_thresh)) & (table[:, 1] > 0) & (table[:, 0].astype(F) >= F(stability_thresh) * table[:, 1].astype(F))


def rank_order(iou, flags):
    """the survivors' candidate indices by iou descending, ties to the smaller index"""
    idx = np.nonzero(flags)[0]
    return idx[np.lexsort((idx, -np.asarray(iou, F)[idx].astype(np.float64)))]


def suppresses(a, b, thresh) -> bool:
    """box a suppresses box b: torchvision's IoU on the inclusive integer coordinates x0, y0, x1, y1, decided as inter > thresh * union in float32"""
    a, b = [int(v) for v in a], [int(v) for v in b]
    area_a, area_b = (a[2] - a[0]) * (a[3] - a[1]), (b[2] - b[0]) * (b[3] - b[1])
    iw, ih = max(0, min(a[2], b[2]) - max(a[0], b[0])), max(0, min(a[3], b[3]) - max(a[1], b[1]))
    inter = iw * ih
    return bool(F(inter) > F(thresh) * F(area_a + area_b - inter))


def nms(boxes, thresh):
    """greedy NMS over boxes int [n, 4] in rank order -> the kept positions. Vectorised over the later boxes, the arithmetic of suppresses()."""
    b = np.asarray(boxes, np.int64).reshape(-1, 4)
    n = len(b)
    area = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    removed = np.zeros(n, bool)
    kept = []
    for i in range(n):
        if removed[i]:
            continue
        kept.append(i)
        r = b[i + 1:]
        iw = np.maximum(0, np.minimum(b[i, 2], r[:, 2]) - np.maximum(b[i, 0], r[:, 0]))
        ih = np.maximum(0, np.minimum(b[i, 3], r[:, 3]) - np.maximum(b[i, 1], r[:, 1]))
        inter = iw * ih
        uni = area[i] + area[i + 1:] - inter
        removed[i + 1:] |= inter.astype(F) > F(thresh) * uni.astype(F)
    return np.array(kept, np.int64)


def rank_nms(table, iou, pred_iou_thresh, stability_thresh, nms_iou_thresh, capacity):
    """-> dict(flags int32 [C], rank int32 [C] (-1 for the filtered), keep int32 [returned], counts (returned, kept))"""
    flags = filters(table, iou, pred_iou_thresh, stability_thresh)
    order = rank_order(iou, flags)
    rank = np.full(len(flags), -1, np.int32)
    rank[order] = np.arange(len(order))
    kept = order[nms(table[order, 2:6], nms_iou_thresh)] if len(order) else order
    returned = min(len(kept), capacity)
    return dict(flags=flags.astype(np.int32), rank=rank, keep=kept[:returned].astype(np.int32), counts=(returned, len(kept)))


def mask_stats(mask):
    """u8 mask [h, w] -> (x, y, w, h, area) of the pixels that are 255; the box is 0, 0, 0, 0 for an empty mask"""
    ys, xs = np.nonzero(mask == 255)
    if not ys.size:
        return 0, 0, 0, 0, 0
    return int(xs.min()), int(ys.min()), int(xs.max() - xs.min() + 1), int(ys.max() - ys.min() + 1), int(ys.size)


def select(logits, iou, w, h, *, pred_iou_thresh, stability_thresh, stability_offset, nms_iou_thresh, capacity, n_planes=3, image_size=1024):
    """The stage on a call's logits [n, 4, M, M] and iou predictions [n, 4]: candidates 3 * prompt + plane ->
    dict(table, stability, cand_iou, flags, rank, keep, counts)"""
    logits, iou = np.asarray(logits), np.asarray(iou, F)
    n, M = logits.shape[0], logits.shape[-1]
    cw, ch = region(*scaled_extent(w, h, image_size), M, image_size)
    table, stability = score_planes(logits[:, :n_planes].reshape(n * n_planes, M, M), cw, ch, stability_offset)
    cand_iou = iou[:, :n_planes].reshape(-1)
    out = rank_nms(table, cand_iou, pred_iou_thresh, stability_thresh, nms_iou_thresh, capacity)
    out.update(table=table, stability=stability, cand_iou=cand_iou)
    return out


def midpoint_thresholds(values):
    """midpoints between adjacent distinct sorted float32 values, as float32, each strictly between its neighbours"""
    v = np.unique(np.asarray(values, F)[np.isfinite(values)])
    mid = ((v[:-1].astype(np.float64) + v[1:]) / 2).astype(F)
    return mid[(mid > v[:-1]) & (mid < v[1:])]


def pick_thresholds(sel_inputs, w, h, stability_offset=1.0):
    """Thresholds for a scenario, taken from its own values: (pred_iou_thresh, stability_thresh, nms_iou_thresh) as midpoints between adjacent sorted
    values such that each filter rejects at least one candidate, at least eight reach NMS, and NMS suppresses at least one and keeps at least two; None
    when the scenario has no such thresholds. sel_inputs = (logits [n, 4, M, M], iou [n, 4])."""
    logits, iou = sel_inputs
    base = select(logits, iou, w, h, pred_iou_thresh=-np.inf, stability_thresh=-np.inf, stability_offset=stability_offset, nms_iou_thresh=1.0, capacity=1 << 30)
    ci, st, table = base["cand_iou"], base["stability"], base["table"]

    def nearest_first(mids, values, q):
        """the midpoints, the one nearest to the q-quantile of the values first: a threshold in the middle of its range holds on a neighbouring run too"""
        return mids[np.argsort(np.abs(mids - np.quantile(np.asarray(values, np.float64), q)), kind="stable")] if len(mids) else mids

    for pt in nearest_first(midpoint_thresholds(ci), ci, 0.3):
        for stt in nearest_first(midpoint_thresholds(st), st[ci > pt], 0.3):
            by_iou = ci > pt
            fl = filters(table, ci, pt, stt)
            if not ((~by_iou).any() and (by_iou & ~fl).any() and fl.sum() >= 8):
                continue
            order = rank_order(ci, fl)
            boxes = table[order, 2:6].astype(np.float64)
            ious = []
            for i in range(len(order)):
                for j in range(i + 1, len(order)):
                    a, b = boxes[i], boxes[j]
                    inter = max(0.0, min(a[2], b[2]) - max(a[0], b[0])) * max(0.0, min(a[3], b[3]) - max(a[1], b[1]))
                    uni = (a[2] - a[0]) * (a[3] - a[1]) + (b[2] - b[0]) * (b[3] - b[1]) - inter
                    if uni > 0:
                        ious.append(inter / uni)
            if not ious:
                continue
            for nt in nearest_first(midpoint_thresholds(np.array(ious, F)), ious, 0.5):
                if not 0 <= nt <= 1:
                    continue
                kept = nms(table[order, 2:6], nt)
                if len(kept) >= 2 and len(kept) < len(order):
                    return float(pt), float(stt), float(nt)
    return None


# ---- the model-level scenario of tests/test_gpu_sam_autogen.py, and of its CPU check in tests/test_sam_select_ref_cpu.py ---------------------------------
SCENARIO_IMAGE_SEED, SCENARIO_ENCODER_SEED, SCENARIO_DECODER_SEED = 31, 2, 11  # the image and the model of tests/test_gpu_sam_prompts.py
SCENARIO_BIAS_SHIFT = 0.7
SCENARIO_BOXES = [[200, 120, 640, 900], [600, 100, 900, 300]]


def scenario_prompts(w=1024, h=1024):
    """a 4 x 4 point grid (the formula of vision.sam_point_grid) plus two boxes: 18 prompts, chunks of 8 + 8 + 2 at chunk 8"""
    xs, ys = ((np.arange(4) + 0.5) * w / 4).astype(int), ((np.arange(4) + 0.5) * h / 4).astype(int)
    return [[int(x), int(y)] for y in ys for x in xs] + [list(b) for b in SCENARIO_BOXES]


def scenario_decoder_state_dict():
    """The synthetic decoder (seed 11) with the last bias of its four hypernetwork MLPs lowered by SCENARIO_BIAS_SHIFT. As it is, that decoder's logits are
    noise with a third of them positive: the box of the positive logits is the whole plane for every candidate, all box IoUs are 1 and NMS keeps exactly
    one, whatever the thresholds (the CPU check asserts this of the oracle). The shift adds -0.7 x (the sum of a pixel's 32 upscaled features, mostly
    positive behind their GELU) to every logit: positives become rare, the boxes differ, and thresholds with the four conditions exist."""
    from visioncpp_amd import synth
    sd = synth.sam_decoder_state_dict(SCENARIO_DECODER_SEED)
    keys = [k for k in sd if "output_hypernetworks_mlps" in k and k.endswith("layers.2.bias")]
    assert len(keys) == 4
    for k in keys:
        sd[k] = (sd[k] - F(SCENARIO_BIAS_SHIFT)).astype(F)
    return sd


def scenario_conditions(sel, pred_iou_thresh):
    """the figures behind the four conditions a model-level scenario must meet, of a select() result (its capacity above the kept count)"""
    flags = sel["flags"].astype(bool)
    with np.errstate(invalid="ignore"):
        by_iou = sel["cand_iou"] > F(pred_iou_thresh)
    n_nms = int(flags.sum())
    return dict(rejected_by_iou=int((~by_iou).sum()), rejected_by_stability=int((by_iou & ~flags).sum()), reached_nms=n_nms, kept=int(sel["counts"][1]),
                suppressed=n_nms - int(sel["counts"][1]))


def assert_scenario(c):
    """each filter rejects at least one candidate, at least eight reach NMS, NMS suppresses at least one and keeps at least two"""
    assert c["rejected_by_iou"] >= 1 and c["rejected_by_stability"] >= 1 and c["reached_nms"] >= 8 and c["suppressed"] >= 1 and c["kept"] >= 2, c

"""tests/sam_select_ref.py pinned without a device, on independent code: the stability score and the box against torch formulations of SAM's
calculate_stability_score and batched_mask_to_box in float64, NMS against a separately written float64 greedy loop (and torchvision.ops.nms where it is
installed), the rank on ties, the capacity cut, the mask records; the argument refusals of the C entries that need no device; and the scenario of
tests/test_gpu_sam_autogen.py with the oracle's own encoder and decoder: thresholds with the four conditions exist for it."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import sam_select_cases as SC
from tests import sam_select_ref as R

F = np.float32


# ---- SAM's own formulations (segment_anything/utils/amg.py), written out in torch float64 ---------------------------------------------------------------
def _sam_stability_score(masks: torch.Tensor, mask_threshold: float, threshold_offset: float) -> torch.Tensor:
    intersections = (masks > (mask_threshold + threshold_offset)).sum(-1, dtype=torch.int64).sum(-1, dtype=torch.int64)
    unions = (masks > (mask_threshold - threshold_offset)).sum(-1, dtype=torch.int64).sum(-1, dtype=torch.int64)
    return intersections.to(torch.float64) / unions.to(torch.float64)


def _sam_mask_to_box(masks: torch.Tensor) -> torch.Tensor:
    """bool [C, h, w] -> XYXY int64 [C, 4], [0, 0, 0, 0] for an empty mask"""
    h, w = masks.shape[-2:]
    in_height, _ = torch.max(masks, dim=-1)
    in_height_coords = in_height * torch.arange(h)[None, :]
    bottom, _ = torch.max(in_height_coords, dim=-1)
    in_height_coords = in_height_coords + h * (~in_height)
    top, _ = torch.min(in_height_coords, dim=-1)
    in_width, _ = torch.max(masks, dim=-2)
    in_width_coords = in_width * torch.arange(w)[None, :]
    right, _ = torch.max(in_width_coords, dim=-1)
    in_width_coords = in_width_coords + w * (~in_width)
    left, _ = torch.min(in_width_coords, dim=-1)
    empty = (right < left) | (bottom < top)
    out = torch.stack([left, top, right, bottom], dim=-1)
    return out * (~empty).unsqueeze(-1)


@pytest.mark.parametrize("M,cw,ch,off", [(16, 16, 16, 1.0), (24, 13, 7, 1.0), (24, 1, 1, 0.5), (64, 40, 64, 0.0), (256, 256, 192, 1.0)])
def test_scores_and_boxes_are_sams(M, cw, ch, off):
    planes = SC.score_planes(M, 3, 3, seed=1).reshape(9, M, M)
    special = SC.special_planes(M, cw, ch, off)
    planes = np.concatenate([planes, np.stack(list(special.values()))])
    table, stab = R.score_planes(planes, cw, ch, off)
    t = torch.from_numpy(planes[:, :ch, :cw].astype(np.float64))
    with np.errstate(invalid="ignore"):
        want_stab = _sam_stability_score(t, 0.0, off).numpy()
    want_box = _sam_mask_to_box(t > 0).numpy()
    np.testing.assert_array_equal(table[:, 2:], want_box)
    uni = table[:, 1]
    assert (uni == 0).any() and (uni > 0).any()  # SAM divides 0 by 0 there; this stage defines the score as 0 and filters the candidate
    np.testing.assert_allclose(stab[uni > 0], want_stab[uni > 0], rtol=2 ** -23, atol=0)
    assert (stab[uni == 0] == 0).all() and stab.dtype == F and table.dtype == np.int32
    names = list(special)
    row = lambda n: table[9 + names.index(n)]
    np.testing.assert_array_equal(row("all-below"), [0, 0, 0, 0, 0, 0])
    np.testing.assert_array_equal(row("all-above"), [cw * ch, cw * ch, 0, 0, cw - 1, ch - 1])
    np.testing.assert_array_equal(row("corners"), [min(4, cw * ch), min(4, cw * ch), 0, 0, cw - 1, ch - 1])
    np.testing.assert_array_equal(row("outside-only"), [0, 0, 0, 0, 0, 0])
    np.testing.assert_array_equal(row("one-pixel")[2:], [cw // 2, ch // 2, cw // 2, ch // 2])
    e = row("exactly-at")  # off, -off, 0, -0 in turn: a value AT a comparison does not pass it
    vals = planes[9 + names.index("exactly-at"), :ch, :cw].astype(np.float64)
    assert e[0] == (vals > off).sum() and e[1] == (vals > -off).sum() and (off == 0 or e[0] == 0)


def _greedy_f64(boxes, thresh):
    """greedy NMS written separately: python floats (float64), a division, one pair at a time"""
    kept = []
    for j, bj in enumerate(boxes):
        ok = True
        for i in kept:
            bi = boxes[i]
            iw = max(0.0, float(min(bi[2], bj[2])) - float(max(bi[0], bj[0])))
            ih = max(0.0, float(min(bi[3], bj[3])) - float(max(bi[1], bj[1])))
            inter = iw * ih
            union = float((bi[2] - bi[0]) * (bi[3] - bi[1])) + float((bj[2] - bj[0]) * (bj[3] - bj[1])) - inter
            if union > 0 and inter / union > thresh:
                ok = False
                break
        if ok:
            kept.append(j)
    return kept


def _pair_ious(boxes):
    b = np.asarray(boxes, np.float64)
    area = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    iw = np.maximum(0, np.minimum(b[:, None, 2], b[None, :, 2]) - np.maximum(b[:, None, 0], b[None, :, 0]))
    ih = np.maximum(0, np.minimum(b[:, None, 3], b[None, :, 3]) - np.maximum(b[:, None, 1], b[None, :, 1]))
    inter = iw * ih
    uni = area[:, None] + area[None, :] - inter
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(uni > 0, inter / uni, 0.0)


SMALL = [c for c in SC.RANK_NMS_CASES if len(c["table"]) <= 130]


@pytest.mark.parametrize("case", SMALL, ids=lambda c: c["id"])
def test_rank_and_nms_against_a_float64_greedy_loop(case):
    table, iou = case["table"], case["iou"]
    got = R.rank_nms(table, iou, case["pred_iou_thresh"], case["stability_thresh"], case["nms_iou_thresh"], case["capacity"])
    # the filters and the order, written out one candidate at a time
    survivors = [c for c in range(len(iou)) if iou[c] > F(case["pred_iou_thresh"]) and table[c, 1] > 0 and table[c, 0] / table[c, 1] >= case["stability_thresh"]]
    order = sorted(survivors, key=lambda c: (-float(iou[c]), c))
    np.testing.assert_array_equal(np.nonzero(got["flags"])[0], survivors)
    np.testing.assert_array_equal([got["rank"][c] for c in order], np.arange(len(order)))
    assert (got["rank"][got["flags"] == 0] == -1).all()
    boxes = table[order, 2:]
    nt = case["nms_iou_thresh"]
    if len(order) > 1 and case["id"] not in ("iou-at-threshold", "degenerate"):  # the comparison needs inputs where no IoU lies within 1e-6 of the threshold
        ious = _pair_ious(boxes)[np.triu_indices(len(order), 1)]
        assert np.abs(ious - nt).min() > 1e-6, np.abs(ious - nt).min()
    want = [order[k] for k in _greedy_f64(boxes, nt)]
    assert got["counts"] == (min(len(want), case["capacity"]), len(want))
    np.testing.assert_array_equal(got["keep"], want[: case["capacity"]])
    try:
        from torchvision.ops import nms as tv_nms
    except Exception:
        return
    if len(order):
        keep = tv_nms(torch.from_numpy(boxes.astype(np.float64)), torch.from_numpy(iou[order].astype(np.float64)), float(nt)).numpy()
        scores = iou[order]
        if len(np.unique(scores)) == len(scores):  # torchvision's order among equal scores is its sort's
            np.testing.assert_array_equal([order[k] for k in keep], want)


def test_named_cases_decide_as_stated():
    cases = {c["id"]: c for c in SC.RANK_NMS_CASES}
    run = lambda c: R.rank_nms(c["table"], c["iou"], c["pred_iou_thresh"], c["stability_thresh"], c["nms_iou_thresh"], c["capacity"])
    np.testing.assert_array_equal(run(cases["chain"])["keep"], [1, 0])             # A = 1, B = 2 falls to A, C = 0 survives
    assert R.suppresses([0, 0, 20, 10], [10, 0, 30, 10], 0.3) and R.suppresses([10, 0, 30, 10], [20, 0, 40, 10], 0.3) and not R.suppresses([0, 0, 20, 10], [20, 0, 40, 10], 0.3)
    np.testing.assert_array_equal(run(cases["iou-at-threshold"])["keep"], [0, 1])  # inter 2, union 4 at 0.5: strictly greater is asked
    np.testing.assert_array_equal(run(cases["iou-above-threshold"])["keep"], [0])
    d = run(cases["degenerate"])                                                 # zero areas: inter 0 > 0 * union never holds
    assert d["counts"] == (6, 6)
    np.testing.assert_array_equal(d["keep"], [3, 0, 1, 2, 5, 4])
    for name in ("all-fail-iou", "all-fail-stability", "all-nan"):
        r = run(cases[name])
        assert r["counts"] == (0, 0) and len(r["keep"]) == 0 and not r["flags"].any() and (r["rank"] == -1).all()
    r = run(cases["nan-and-inf"])                                                # +inf ranks first, NaN and -inf fail, the tie goes to the smaller index
    np.testing.assert_array_equal(r["keep"], [2, 1, 4])
    np.testing.assert_array_equal(r["flags"], [0, 1, 1, 0, 1, 0])
    r = run(cases["equal-scores-65"])
    np.testing.assert_array_equal(r["keep"], [0, 1])
    np.testing.assert_array_equal(r["rank"], np.arange(65))
    r = run(cases["capacity-1"])
    assert r["counts"] == (1, 130) and list(r["keep"]) == [129]
    r = run(cases["identical-4097"])
    assert r["counts"] == (1, 1) and list(r["keep"]) == [0]
    r = run(cases["disjoint-16384"])
    assert r["counts"] == (300, 16384)
    order = R.rank_order(cases["disjoint-16384"]["iou"], np.ones(16384, bool))
    np.testing.assert_array_equal(r["keep"], order[:300])
    assert order[0] == 4098 and order[1] == 4098 + 4099  # the largest score, its ties by index
    cut = cases["mixed-130-cut"]
    full = R.rank_nms(cut["table"], cut["iou"], cut["pred_iou_thresh"], cut["stability_thresh"], cut["nms_iou_thresh"], 1000)
    got = run(cut)
    assert got["counts"] == (cut["capacity"], full["counts"][1]) and full["counts"][1] > cut["capacity"]
    np.testing.assert_array_equal(got["keep"], full["keep"][: cut["capacity"]])


def test_region_extent_and_mask_records():
    assert R.scaled_extent(1024, 1024) == (1024, 1024) and R.region(1024, 1024) == (256, 256)
    assert R.scaled_extent(640, 480) == (1024, 768) and R.region(1024, 768) == (256, 192)
    sw, sh = R.scaled_extent(333, 517)
    assert (sw, sh) == (660, 1024) and R.region(sw, sh) == (165, 256)
    assert R.region(1021, 3) == (256, 1)  # a part of a logit counts as the logit
    m = np.zeros((5, 9), np.uint8)
    assert R.mask_stats(m) == (0, 0, 0, 0, 0)
    m[1, 2] = m[3, 7] = 255
    m[4, 8] = 254  # not a mask value: not counted
    assert R.mask_stats(m) == (2, 1, 6, 3, 2)
    assert R.mask_stats(np.full((3, 4), 255, np.uint8)) == (0, 0, 4, 3, 12)


def test_select_numbers_candidates_by_prompt_then_plane():
    rng = np.random.default_rng(3)
    logits = (rng.standard_normal((5, 4, 16, 16)) * 2).astype(np.float16)
    iou = rng.random((5, 4)).astype(F)
    iou[:, 3] = 9.0  # the fourth plane is no candidate, whatever it predicts
    s = R.select(logits, iou, 64, 64, pred_iou_thresh=0.2, stability_thresh=0.1, stability_offset=1.0, nms_iou_thresh=1.0, capacity=4, image_size=64)
    assert s["table"].shape == (15, 6) and s["counts"][0] == 4
    t7, st7 = R.score_planes(logits[2, 1][None], 16, 16, 1.0)
    np.testing.assert_array_equal(s["table"][7], t7[0])
    assert s["cand_iou"][7] == iou[2, 1] and s["stability"][7] == st7[0]
    assert s["cand_iou"][s["keep"][0]] == s["cand_iou"][s["flags"] == 1].max() < 9.0


def test_c_entries_refuse_bad_arguments_without_a_device():
    from visioncpp_amd import _lib as L
    api = L.get_lib()
    d = (C.c_float * 4)()
    assert api.visp_sam_generate_defaults(d) == 1 and [round(float(v), 6) for v in d] == [0.88, 0.95, 1.0, 0.7]
    assert api.visp_sam_generate_defaults(None) == 0 and b"null" in api.visp_get_last_error()
    p, k = np.zeros((2, 4), np.int32), np.full(2, 2, np.int32)
    big_p, big_k = np.zeros((5462, 4), np.int32), np.full(5462, 2, np.int32)
    out = np.zeros(64, np.uint8).ctypes.data
    nan = float("nan")
    good = (0.88, 0.95, 1.0, 0.7, 4)
    for args, n, pp, kk, msg in [
        ((nan, 0.95, 1.0, 0.7, 4), 2, p, k, b"NaN"), ((0.88, nan, 1.0, 0.7, 4), 2, p, k, b"NaN"), ((0.88, 0.95, nan, 0.7, 4), 2, p, k, b"NaN"),
        ((0.88, 0.95, 1.0, nan, 4), 2, p, k, b"NaN"), ((0.88, 0.95, 1.0, 1.5, 4), 2, p, k, b"outside [0, 1]"), ((0.88, 0.95, 1.0, -0.1, 4), 2, p, k, b"outside [0, 1]"),
        ((0.88, 0.95, -0.5, 0.7, 4), 2, p, k, b"below 0"), ((0.88, 0.95, 1.0, 0.7, 0), 2, p, k, b"capacity"), (good, 0, p, k, b"empty batch"),
        (good, 5462, big_p, big_k, b"at most 5461"), (good, 2, None, k, b"null"), (good, 2, p, None, b"null"),
    ]:
        pa, ka = (pp.ctypes.data if pp is not None else None), (kk.ctypes.data if kk is not None else None)
        assert api.visp_sam_generate_masks_device(None, pa, ka, n, *args, out, out, out, out, None) == 0
        assert msg in api.visp_get_last_error(), (msg, api.visp_get_last_error())
        assert api.visp_sam_generate_masks_host(None, pa, ka, n, *args, out, out, out, out) == 0
        assert msg in api.visp_get_last_error(), (msg, api.visp_get_last_error())
    # everything in order but the handle
    assert api.visp_sam_generate_masks_device(None, p.ctypes.data, k.ctypes.data, 2, *good, out, out, out, out, None) == 0
    assert b"model handle is null" in api.visp_get_last_error()
    # the launchers' host-side refusals that come before any device call
    assert api.vx_sam_rank_nms_workspace_bytes(0) == 0 and api.vx_sam_rank_nms_workspace_bytes(16385) == 0
    assert api.vx_sam_rank_nms_workspace_bytes(16384) >= 16384 * 256 * 8 and api.vx_sam_rank_nms_workspace_bytes(1) >= 8


@pytest.fixture(scope="module")
def oracle_runs():
    """the scenario through the oracle's own encoder and decoder: (logits f16 [18, 4, 256, 256], iou [18, 4]) for the synthetic decoder as it is and shifted"""
    from oracle import oracle as O
    from visioncpp_amd import synth
    cfg = synth.TINYVIT_5M
    enc_sd = synth.tinyvit_state_dict(cfg, R.SCENARIO_ENCODER_SEED)
    img = synth.images(1, 1024, 1024, seed=R.SCENARIO_IMAGE_SEED)[0]
    mean, std = np.array([0.485, 0.456, 0.406], F), np.array([0.229, 0.224, 0.225], F)
    x = (img.astype(F) / F(255.0) - mean) / std
    out, emb = {}, None
    for name, dec_sd in (("as-it-is", synth.sam_decoder_state_dict(R.SCENARIO_DECODER_SEED)), ("shifted", R.scenario_decoder_state_dict())):
        tensors, conv2d = synth.mobile_sam_gguf_tensors(enc_sd, dec_sd)
        om = O.Model(tensors, conv2d, "whcn")
        if emb is None:  # the encoder is the same in both
            emb = O.tinyvit_encode(om, O.tinyvit_params(cfg.img_size, cfg.layers()), x)
        runs = [O.sam_compute(om, emb, 1024, 1024, p, return_all=True) for p in R.scenario_prompts()]
        out[name] = (np.stack([r[2] for r in runs]).astype(np.float16), np.stack([r[1] for r in runs]))
    return out


def test_scenario_has_thresholds_with_the_four_conditions(oracle_runs):
    """For tests/test_gpu_sam_autogen.py: with the oracle's own encoder and decoder on the same image and prompts, thresholds taken as midpoints between
    adjacent sorted values exist such that each filter rejects a candidate, at least eight reach NMS, and NMS suppresses one and keeps two. The synthetic
    decoder as it is has none (every box is the whole plane): the reason the scenario lowers four biases."""
    from visioncpp_amd import vision
    assert R.scenario_prompts() == [list(p) for p in vision.sam_point_grid(4, 1024, 1024)] + R.SCENARIO_BOXES
    plain = R.select(*oracle_runs["as-it-is"], 1024, 1024, pred_iou_thresh=-np.inf, stability_thresh=-np.inf, stability_offset=1.0, nms_iou_thresh=1.0, capacity=1 << 20)
    assert (plain["table"][:, 2:] == [0, 0, 255, 255]).all() and R.pick_thresholds(oracle_runs["as-it-is"], 1024, 1024) is None
    logits, iou = oracle_runs["shifted"]
    picked = R.pick_thresholds((logits, iou), 1024, 1024)
    assert picked is not None
    pt, st, nt = picked
    sel = R.select(logits, iou, 1024, 1024, pred_iou_thresh=pt, stability_thresh=st, stability_offset=1.0, nms_iou_thresh=nt, capacity=1 << 20)
    c = R.scenario_conditions(sel, pt)
    print(f"thresholds {picked}: {c}")
    R.assert_scenario(c)
    assert len(np.unique(sel["table"][:, 2:], axis=0)) >= 8  # the boxes differ

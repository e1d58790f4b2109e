"""tests/sam_regions_ref.py pinned without a GPU. Its labelling against scipy.ndimage.label with the 3 x 3 structure (8-connectivity, which is how SAM calls
cv2.connectedComponentsWithStats): the components, their sizes and their first-pixel order. Its remove_small_regions and postprocess against a literal
transcription of SAM's remove_small_regions / postprocess_small_regions (segment_anything/utils/amg.py, automatic_mask_generator.py) with that labelling in
cv2's place and a separately written greedy NMS loop for torchvision's. The named cases do what their names say. The new C entries refuse what needs no
device to refuse. And the scenario of tests/test_gpu_sam_regions.py, with the oracle's own encoder and decoder, has a min_region_area with the three conditions."""
import numpy as np
import pytest
from scipy import ndimage

from tests import sam_regions_cases as SC
from tests import sam_regions_ref as RR
from tests import sam_select_ref as R

EIGHT = np.ones((3, 3), int)
CASES = SC.named_cases()


# ---- SAM, transcribed -------------------------------------------------------------------------------------------------------------------------------------

def _sam_remove_small_regions(mask: np.ndarray, area_thresh: float, mode: str):
    """amg.py remove_small_regions on a bool mask; cv2.connectedComponentsWithStats(working_mask, 8) -> scipy's label with the 3 x 3 structure (label 0 is the
    rest, labels from 1 in order of the first pixel, as cv2 numbers them)"""
    assert mode in ["holes", "islands"]
    correct_holes = mode == "holes"
    working_mask = (correct_holes ^ mask).astype(np.uint8)
    regions, n_labels = ndimage.label(working_mask, structure=EIGHT)
    n_labels += 1
    sizes = np.bincount(regions.reshape(-1), minlength=n_labels)[1:]
    small_regions = [i + 1 for i, s in enumerate(sizes) if s < area_thresh]
    if len(small_regions) == 0:
        return mask, False
    fill_labels = [0] + small_regions
    if not correct_holes:
        fill_labels = [i for i in range(n_labels) if i not in fill_labels]
        if len(fill_labels) == 0:
            fill_labels = [int(np.argmax(sizes)) + 1]
    mask = np.isin(regions, fill_labels)
    return mask, True


def _flipped(before, after, sam_changed):
    """The `changed` of the specification: a pixel flipped. SAM's own flag says "a small region was found", which differs in exactly one situation: every island
    is small and the largest, which stays, is the only one -- SAM then reports a change (and scores the mask 0) although it returns the mask as it was."""
    flipped = bool((before != after).any())
    assert flipped == sam_changed or (sam_changed and not flipped and ndimage.label(before, structure=EIGHT)[1] == 1)
    return flipped


def _greedy_nms_f64(boxes, scores, thresh):
    """torchvision.ops.nms written out: by score descending (equal scores by index, the tie torchvision leaves open), IoU on the coordinates as given"""
    b = np.asarray(boxes, np.float64).reshape(-1, 4)
    order = sorted(range(len(b)), key=lambda i: (-scores[i], i))
    keep = []
    for i in order:
        ok = True
        for j in keep:
            iw, ih = max(0.0, min(b[i, 2], b[j, 2]) - max(b[i, 0], b[j, 0])), max(0.0, min(b[i, 3], b[j, 3]) - max(b[i, 1], b[j, 1]))
            inter = iw * ih
            union = (b[i, 2] - b[i, 0]) * (b[i, 3] - b[i, 1]) + (b[j, 2] - b[j, 0]) * (b[j, 3] - b[j, 1]) - inter
            if union > 0 and inter / union > thresh:
                ok = False
                break
        if ok:
            keep.append(i)
    return keep


def _sam_postprocess_small_regions(masks, min_area, nms_thresh):
    """automatic_mask_generator.py postprocess_small_regions on bool masks -> (the kept indices in nms's order, the new masks, the scores)"""
    new_masks, scores = [], []
    for mask in masks:
        filled, changed = _sam_remove_small_regions(mask, min_area, mode="holes")
        unchanged = not _flipped(mask, filled, changed)
        mask, changed = _sam_remove_small_regions(filled, min_area, mode="islands")
        unchanged = unchanged and not _flipped(filled, mask, changed)
        new_masks.append(mask)
        scores.append(float(unchanged))
    boxes = [RR.inclusive_box(np.where(m, 255, 0).astype(np.uint8)) for m in new_masks]  # batched_mask_to_box: inclusive, zeros for an empty mask
    return _greedy_nms_f64(boxes, scores, nms_thresh), new_masks, scores


# ---- the labelling ---------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(CASES))
def test_components_sizes_and_first_pixel_order_are_scipys(name):
    masks, _ = CASES[name]
    for m in masks:
        for fg in (False, True):
            member = (m != 0) == fg
            labels, first, sizes = RR.label_components(member)
            ref, n = ndimage.label(member, structure=EIGHT)
            assert n == len(first) == len(sizes)
            assert ((labels >= 0) == member).all()
            if not n:
                continue
            flat, lab = ref.reshape(-1), labels.reshape(-1)
            ref_first = ndimage.minimum(np.arange(flat.size), flat, index=np.arange(1, n + 1)).astype(np.int64)
            assert (np.diff(ref_first) > 0).all()              # scipy numbers by first pixel, as cv2 does
            assert (first == ref_first).all()                  # the same components in the same order
            assert (sizes == np.bincount(flat, minlength=n + 1)[1:]).all()
            assert (lab[member.reshape(-1)] == ref_first[flat[member.reshape(-1)] - 1]).all()  # every pixel carries its component's first pixel


def test_a_serpentine_through_1024_squared_is_one_component():
    s = SC.serpentine(1024, 1024)
    _, first, sizes = RR.label_components(s != 0)
    assert first.tolist() == [0] and sizes.tolist() == [524799]
    _, first, sizes = RR.label_components(s == 0)
    assert len(sizes) == 512 and sizes[:-1].tolist() == [1023] * 511 and sizes[-1] == 1024


# ---- the masks and the flags -----------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(CASES))
def test_masks_and_flags_are_sams(name):
    masks, min_area = CASES[name]
    for area in sorted({min_area, 1} if masks[0].size > 50000 else {min_area, 0, 1, 2, min_area + 1}):  # the large extents at their own value only
        for mode, name_of in ((RR.HOLES, "holes"), (RR.ISLANDS, "islands")):
            got, changed = RR.remove_small_regions(masks, area, mode)
            for k, m in enumerate(masks):
                want, ch = _sam_remove_small_regions(m != 0, area, name_of)
                assert ((got[k] != 0) == want).all() and bool(changed[k]) == _flipped(m != 0, want, ch), (name, area, name_of, k)
                assert (got[k][(got[k] != 0) == (m != 0)] == m[(got[k] != 0) == (m != 0)]).all()  # only flipped pixels are written, as 0 or 255
                assert set(np.unique(got[k][(got[k] != 0) != (m != 0)])) <= {0, 255}
        got, changed = RR.remove_small_regions(masks, area, RR.BOTH)
        for k, m in enumerate(masks):
            a, c1 = _sam_remove_small_regions(m != 0, area, "holes")
            b, c2 = _sam_remove_small_regions(a, area, "islands")
            assert ((got[k] != 0) == b).all() and bool(changed[k]) == (_flipped(m != 0, a, c1) or _flipped(a, b, c2)), (name, area, k)
        assert RR.remove_small_regions(masks, area, "both")[0].tobytes() == got.tobytes()
        if area <= 1:
            assert got.tobytes() == masks.tobytes() and not changed.any()


def test_named_cases_do_what_their_names_say():
    got, ch = RR.remove_small_regions(SC.two_equal_small_islands(), 9, RR.ISLANDS)
    assert ch.tolist() == [1] and (got[2:4, 3:5] == 255).all() and int((got != 0).sum()) == 4
    m = SC.hole_between_islands()
    both, ch = RR.remove_small_regions(m, 20, RR.BOTH)
    assert ch.tolist() == [1] and (both[0:5] == 255).all() and (both[5:26] == 0).all() and (both[26:] == 255).all()
    isl, _ = RR.remove_small_regions(m, 20, RR.ISLANDS)
    assert (isl[0:26] == 0).all() and (isl[26:] == 255).all()       # the order of the steps matters
    got, ch = RR.remove_small_regions(SC.hole_at_border(), 5, RR.HOLES)
    assert ch.tolist() == [1] and (got == 255).all()                # no exemption at the border
    got, _ = RR.remove_small_regions(SC.exact_area(7), 7, RR.BOTH)
    assert (got[1, 1:8] == 255).all() and (got[3] == 0).all() and (got[7, 2:9] == 0).all() and (got[9] == 255).all()  # exactly min_area stays
    assert len(RR.label_components(SC.checkerboard(67, 37) != 0)[1]) == 1 and len(RR.label_components(SC.checkerboard(67, 37) == 0)[1]) == 1
    assert len(RR.label_components(SC.diagonal(98, 98) != 0)[1]) == 1 and len(RR.label_components(SC.diagonal(98, 98) == 0)[1]) == 1  # 8-connected both: the background crosses it
    empty = np.zeros((5, 5), np.uint8)
    assert RR.remove_small_regions(empty, 3, RR.ISLANDS)[0].tobytes() == empty.tobytes()


# ---- the second NMS ----------------------------------------------------------------------------------------------------------------------------------------------------

def _stage_one(seed, k=9, w=90, h=70):
    """k masks that overlap in groups, with speckle: blobs at a few centres plus noise pixels and pinholes"""
    rng = np.random.default_rng(seed)
    masks = np.zeros((k, h, w), np.uint8)
    centres = [(20, 20), (60, 40), (30, 50)]
    for i in range(k):
        cx, cy = centres[i % 3]
        dx, dy, r = rng.integers(-2, 3), rng.integers(-2, 3), rng.integers(8, 13)
        masks[i, max(cy + dy - r, 0):cy + dy + r, max(cx + dx - r, 0):cx + dx + r] = 255
        if i % 4:  # three of four carry speckle; the others are clean and stay unchanged
            noise = rng.random((h, w)) < 0.01
            masks[i][noise] ^= 255
    info = np.zeros((k, 8), np.int32)
    info[:, 0], info[:, 1] = np.arange(k), np.arange(k) % 3
    for i in range(k):
        info[i, 2:7] = R.mask_stats(masks[i])
    info_f = np.stack([np.sort(rng.random(k).astype(np.float32))[::-1], rng.random(k).astype(np.float32)], axis=1)
    return masks, info, info_f


@pytest.mark.parametrize("seed,thresh", [(1, 0.5), (2, 0.7), (3, 0.3), (4, 0.6)])
def test_postprocess_is_sams_order_and_content(seed, thresh):
    masks, info, info_f = _stage_one(seed)
    post = RR.postprocess(masks, info, info_f, 6, thresh)
    keep, new_masks, scores = _sam_postprocess_small_regions([m != 0 for m in masks], 6, thresh)
    assert post["keep"].tolist() == keep
    assert 0 < sum(scores) < len(scores) and len(keep) < len(masks)  # some change, some do not, some are removed
    assert post["changed"].tolist() == [int(s == 0.0) for s in scores]
    for out, i in zip(post["masks"], keep):
        assert ((out != 0) == new_masks[i]).all()
    assert post["info_i32"][:, 7].tolist() == [int(scores[i] == 0.0) for i in keep] and post["info_i32"][:, 0].tolist() == keep
    assert post["info_f32"].tobytes() == info_f[keep].tobytes()
    for row, out in zip(post["info_i32"], post["masks"]):
        assert tuple(row[2:7]) == R.mask_stats(out)
    flags = post["info_i32"][:, 7]
    assert (np.diff(flags) >= 0).all()                                  # unchanged first, then changed
    for f in (0, 1):
        assert (np.diff(post["info_f32"][flags == f, 0]) <= 0).all()    # each group by predicted iou
    assert post["changed_count"] == int(flags.sum()) and post["removed"] == len(masks) - len(keep)


def test_postprocess_of_nothing_and_of_empty_masks():
    post = RR.postprocess(np.zeros((0, 8, 8), np.uint8), np.zeros((0, 8), np.int32), np.zeros((0, 2), np.float32), 5, 0.7)
    assert len(post["masks"]) == 0 and post["removed"] == 0
    masks = np.zeros((3, 8, 8), np.uint8)
    post = RR.postprocess(masks, np.zeros((3, 8), np.int32), np.zeros((3, 2), np.float32), 5, 0.7)
    assert post["keep"].tolist() == [0, 1, 2]  # boxes [0, 0, 0, 0]: nothing to intersect, nobody is suppressed


# ---- the C entries' refusals that need no device ----------------------------------------------------------------------------------------------------------------------

def test_c_entries_refuse_bad_arguments_without_a_device():
    from visioncpp_amd import _lib as L
    api = L.get_lib()
    buf = np.zeros(256, np.uint8)
    m = buf.ctypes.data
    for args, msg in [((None, 1, 4, 4, 2, 3), b"null"), ((m, 0, 4, 4, 2, 3), b"empty batch"), ((m, -1, 4, 4, 2, 3), b"empty batch"), ((m, 1, 0, 4, 2, 3), b"extent"),
                      ((m, 1, 4, 0, 2, 3), b"extent"), ((m, 1, 4, 4, -1, 3), b"min_area"), ((m, 1, 4, 4, 2, 0), b"unknown mode"), ((m, 1, 4, 4, 2, 4), b"unknown mode")]:
        assert api.visp_image_remove_small_regions_device(*args, None, None, None) == 0
        assert msg in api.visp_get_last_error(), (msg, api.visp_get_last_error())
        assert api.visp_image_remove_small_regions_host(*args, None, None) == 0
        assert msg in api.visp_get_last_error(), (msg, api.visp_get_last_error())
    assert not buf.any()
    p, k = np.zeros((2, 4), np.int32), np.full(2, 2, np.int32)
    out = np.zeros(64, np.uint8).ctypes.data
    for args, n, pp, kk, msg in [((0.88, 0.95, 1.0, 0.7, 4, -1), 2, p, k, b"min_region_area"), ((0.88, 0.95, 1.0, 0.7, 0, 5), 2, p, k, b"capacity"),
                                 ((float("nan"), 0.95, 1.0, 0.7, 4, 5), 2, p, k, b"NaN"), ((0.88, 0.95, 1.0, 1.5, 4, 5), 2, p, k, b"outside [0, 1]"),
                                 ((0.88, 0.95, 1.0, 0.7, 4, 5), 0, p, k, b"empty batch"), ((0.88, 0.95, 1.0, 0.7, 4, 5), 2, None, k, b"null"),
                                 ((0.88, 0.95, 1.0, 0.7, 4, 5), 2, p, k, b"model handle is null"), ((0.88, 0.95, 1.0, 0.7, 4, 0), 2, p, k, b"model handle is null")]:
        pa, ka = (pp.ctypes.data if pp is not None else None), (kk.ctypes.data if kk is not None else None)
        assert api.visp_sam_generate_masks_clean_device(None, pa, ka, n, *args, out, out, out, out, None) == 0
        assert msg in api.visp_get_last_error(), (msg, api.visp_get_last_error())
        assert api.visp_sam_generate_masks_clean_host(None, pa, ka, n, *args, out, out, out, out) == 0
        assert msg in api.visp_get_last_error(), (msg, api.visp_get_last_error())
    assert api.visp_sam_generate_last_split5(None, None) == 0 and api.visp_sam_generate_last_clean_split(None, None) == 0
    # the launcher's workspace query refuses what the launcher refuses
    assert api.vx_mask_regions_workspace_bytes(1024, 1024, 1) >= 8 << 20 and api.vx_mask_regions_workspace_bytes(0, 4, 1) == 0 and api.vx_mask_regions_workspace_bytes(4, 4, 0) == 0
    from visioncpp_amd import vision
    with pytest.raises(ValueError, match="unknown mode"):
        vision.remove_small_regions(np.zeros((4, 4), np.uint8), 3, mode="lakes")
    with pytest.raises(ValueError, match="expected masks"):
        vision.remove_small_regions(np.zeros(4, np.uint8), 3)


# ---- the scenario of tests/test_gpu_sam_regions.py ----------------------------------------------------------------------------------------------------------------------

def test_scenario_has_a_min_region_area_with_the_three_conditions():
    """With the oracle's own encoder and decoder on the scenario's image and prompts, the filters open and the NMS threshold that the selection scenario picks: a
    min_region_area exists at which some first-stage masks change, some do not and the second NMS removes at least one. The scenario's masks are sparse -- most
    are empty --, so the value found is the one the picker tries last, the image's pixel count: masks with any foreground fill up (their background is a small
    hole: no exemption at the border) and suppress each other, empty ones stay."""
    from oracle import oracle as O
    from tests import sam_prompts_ref as PR
    from visioncpp_amd import synth
    F = np.float32
    cfg = synth.TINYVIT_5M
    img = synth.images(1, 1024, 1024, seed=R.SCENARIO_IMAGE_SEED)[0]
    mean, std = np.array([0.485, 0.456, 0.406], F), np.array([0.229, 0.224, 0.225], F)
    tensors, conv2d = synth.mobile_sam_gguf_tensors(synth.tinyvit_state_dict(cfg, R.SCENARIO_ENCODER_SEED), R.scenario_decoder_state_dict())
    om = O.Model(tensors, conv2d, "whcn")
    emb = O.tinyvit_encode(om, O.tinyvit_params(cfg.img_size, cfg.layers()), (img.astype(F) / F(255.0) - mean) / std)
    runs = [O.sam_compute(om, emb, 1024, 1024, p, return_all=True) for p in R.scenario_prompts()]
    logits, iou = np.stack([r[2] for r in runs]).astype(np.float16), np.stack([r[1] for r in runs])
    picked = R.pick_thresholds((logits, iou), 1024, 1024)
    assert picked is not None
    nt = picked[2]
    sel = R.select(logits, iou, 1024, 1024, pred_iou_thresh=-np.inf, stability_thresh=-np.inf, stability_offset=1.0, nms_iou_thresh=nt, capacity=64)
    keep = sel["keep"]
    masks = np.stack([PR.process_mask(logits[c // 3, c % 3].astype(F), 1024, 1024) for c in keep])
    info = np.array([[c // 3, c % 3, *R.mask_stats(masks[k]), 0] for k, c in enumerate(keep)], np.int32)
    info_f = np.stack([sel["cand_iou"][keep], sel["stability"][keep]], axis=1).astype(F)
    area = RR.pick_min_region_area(masks, info, info_f, nt)
    assert area is not None
    post = RR.postprocess(masks, info, info_f, area, nt)
    c = RR.scenario_conditions(post, len(masks))
    print(f"nms_iou_thresh {nt}, {len(masks)} first-stage masks, min_region_area {area}: {c}")
    RR.assert_scenario(c)

"""SAM's remove_small_regions / postprocess_small_regions restated in numpy (csrc/kernels_regions.hip, the min_region_area path of
sam_generate_masks_device): what the device must compute, byte for byte. The labelling is this file's own: runs of a row, a union-find over the
runs of adjacent rows, 8-connectivity; no scipy. tests/test_sam_regions_ref_cpu.py pins it on independent code."""
from __future__ import annotations

import numpy as np

from tests import sam_select_ref as R

HOLES, ISLANDS, BOTH = 1, 2, 3
MODES = {"holes": HOLES, "islands": ISLANDS, "both": BOTH}


def _runs(member):
    """the maximal runs of True of a bool [h, w] in row-major order -> (row, first x, last x) int64 arrays"""
    h, w = member.shape
    pad = np.zeros((h, w + 2), np.int8)
    pad[:, 1:-1] = member
    d = np.diff(pad, axis=1)
    ry, rs = np.nonzero(d == 1)
    _, re = np.nonzero(d == -1)
    return ry, rs, re - 1


def label_components(member):
    """bool [h, w] -> (labels int32 [h, w], first int64 [c], sizes int64 [c]). The label of a pixel is the smallest row-major pixel index of its
    8-connected component, -1 outside the set; `first` holds the components' labels ascending (cv2's label order), `sizes` their pixel counts."""
    member = np.asarray(member, bool)
    h, w = member.shape
    ry, rs, re = _runs(member)
    n = len(ry)
    parent = list(range(n))

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a

    row_start = np.searchsorted(ry, np.arange(h + 1))
    rsl, rel = rs.tolist(), re.tolist()
    for y in range(1, h):
        a, a_end, b, b_end = row_start[y - 1], row_start[y], row_start[y], row_start[y + 1]
        while a < a_end and b < b_end:  # runs touch iff their x ranges, widened by one, overlap
            if rsl[a] <= rel[b] + 1 and rsl[b] <= rel[a] + 1:
                ra, rb = find(a), find(b)
                if ra != rb:
                    parent[max(ra, rb)] = min(ra, rb)  # the smaller run id holds the smaller first pixel
            if rel[a] < rel[b]:
                a += 1
            else:
                b += 1
    root = np.array([find(i) for i in range(n)], np.int64)
    first_of_run = ry * w + rs
    length = re - rs + 1
    labels = np.full(h * w, -1, np.int32)
    if n:
        idx = np.repeat(first_of_run - np.cumsum(length) + length, length) + np.arange(length.sum())
        labels[idx] = np.repeat(first_of_run[root], length)
    roots = np.unique(root)
    sizes = np.bincount(root, weights=length, minlength=n).astype(np.int64)[roots] if n else np.zeros(0, np.int64)
    return labels.reshape(h, w), first_of_run[roots] if n else np.zeros(0, np.int64), sizes


def _step(mask, min_area, islands):
    """one step on a u8 mask in place -> whether a pixel flipped"""
    labels, first, sizes = label_components((mask != 0) == islands)
    small = sizes < min_area
    if islands and len(sizes) and small.all():
        small[int(np.argmax(sizes))] = False  # argmax takes the first of equal ones: the component whose first pixel comes first
    flip = np.isin(labels, first[small]) if small.any() else np.zeros(mask.shape, bool)
    mask[flip] = 0 if islands else 255
    return bool(flip.any())


def remove_small_regions(masks, min_area: int, mode=BOTH):
    """u8 [n, h, w] or [h, w] -> (masks, changed int32 [n]) by the semantics of the issue: holes (small background components become 255, none exempt),
    then islands (small foreground components become 0; where every one is small the largest stays). Only flipped pixels change."""
    mode = MODES.get(mode, mode)
    assert mode in (HOLES, ISLANDS, BOTH) and min_area >= 0
    m = np.array(masks, np.uint8, copy=True)
    out = m.reshape((-1,) + m.shape[-2:])
    changed = np.zeros(len(out), np.int32)
    for k in range(len(out)):
        if mode & HOLES:
            changed[k] |= _step(out[k], min_area, False)
        if mode & ISLANDS:
            changed[k] |= _step(out[k], min_area, True)
    return m, changed


def inclusive_box(mask):
    """[x0, y0, x1, y1] of the pixels that are 255, in image pixels; [0, 0, 0, 0] for an empty mask"""
    x, y, w, h, area = R.mask_stats(mask)
    return [x, y, x + w - 1, y + h - 1] if area else [0, 0, 0, 0]


def second_nms(boxes, changed, nms_iou_thresh):
    """the second NMS of postprocess_small_regions over k masks in first-stage rank order: score 1 for an unchanged mask, 0 for a changed one, equal
    scores in first-stage order -> the kept positions in output order (unchanged first, then changed, each in first-stage order)"""
    changed = np.asarray(changed).astype(bool)
    order = np.concatenate([np.nonzero(~changed)[0], np.nonzero(changed)[0]]).astype(np.int64)
    if not len(order):
        return order
    return order[R.nms(np.asarray(boxes, np.int64)[order], nms_iou_thresh)]


def postprocess(masks, info_i32, info_f32, min_region_area, nms_iou_thresh):
    """The min_region_area path on a call's first-stage output (the k returned masks [k, h, w] with their rows [k, 8] and [k, 2]) ->
    dict(masks, info_i32, info_f32, changed_count, removed): what the cleaning entry returns, in its order."""
    masks, info_i32, info_f32 = np.asarray(masks), np.asarray(info_i32), np.asarray(info_f32)
    k = len(masks)
    cleaned, changed = remove_small_regions(masks, min_region_area, BOTH) if k else (masks.copy(), np.zeros(0, np.int32))
    rows = info_i32.copy()
    for i in range(k):
        rows[i, 2:7] = R.mask_stats(cleaned[i])
        rows[i, 7] = changed[i]
    keep = second_nms([inclusive_box(c) for c in cleaned], changed, nms_iou_thresh)
    return dict(masks=cleaned[keep], info_i32=rows[keep], info_f32=info_f32[keep], changed_count=int(changed[keep].sum()), removed=k - len(keep), keep=keep,
                changed=changed)


def min_component_size(mask):
    """the pixel count of the smallest component of a u8 mask, background and foreground alike: remove_small_regions changes the mask at every min_area above it
    (but for a mask whose only small component is its only island, which stays)"""
    sizes = [label_components((mask != 0) == fg)[2] for fg in (False, True)]
    return int(min(s.min() for s in sizes if len(s)))


def scenario_conditions(post, k):
    """the figures behind the three conditions a model-level scenario must meet, of a postprocess() result over k first-stage masks"""
    n_changed = int(post["changed"].sum())
    return dict(changed=n_changed, unchanged=k - n_changed, removed=int(post["removed"]))


def assert_scenario(c):
    """some masks change, some do not, and the second NMS removes at least one"""
    assert c["changed"] >= 1 and c["unchanged"] >= 1 and c["removed"] >= 1, c


def pick_min_region_area(masks, info_i32, info_f32, nms_iou_thresh, tries=8):
    """A min_region_area for a scenario, taken from its own first-stage masks, at which some masks change, some do not and the second NMS removes at least one;
    None when no candidate does. Candidates: one above the smallest component of some mask and not above that of another (the `tries` smallest such values),
    then the pixel count of the image: no component is exempt for touching the border, so at that value a mask with any foreground loses its whole
    background and becomes full, while an empty mask, whose background is the image, stays as it is -- and full masks suppress each other."""
    masks = np.asarray(masks)
    smallest = sorted({min_component_size(m) for m in masks})
    for area in [t + 1 for t in smallest[:-1][:tries]] + [int(masks.shape[-1] * masks.shape[-2])]:
        c = scenario_conditions(postprocess(masks, info_i32, info_f32, area, nms_iou_thresh), len(masks))
        if c["changed"] >= 1 and c["unchanged"] >= 1 and c["removed"] >= 1:
            return area
    return None

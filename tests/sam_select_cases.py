"""Cases of the selection kernels (csrc/kernels_samselect.hip) shared by tests/test_sam_select_ref_cpu.py, which holds the reference to independent code on
them, and tests/test_gpu_sam_select_kernels.py, which holds the device to the reference. Plain numpy; built once at import, small except where a size
is the point (4097 and 16384 candidates)."""
from __future__ import annotations

import numpy as np

F = np.float32
PASS = dict(pred_iou_thresh=0.5, stability_thresh=0.5)  # a row with iou 0.9, inter 3, uni 4 passes both


def _table(boxes, inter=3, uni=4):
    b = np.asarray(boxes, np.int32).reshape(-1, 4)
    t = np.zeros((len(b), 6), np.int32)
    t[:, 0], t[:, 1], t[:, 2:] = inter, uni, b
    return t


def _disjoint(n):
    """n boxes of 2 x 2 pixels on a 128 x 128 grid of cells: no two share a pixel"""
    i = np.arange(n)
    x, y = 2 * (i % 128), 2 * (i // 128)
    return np.stack([x, y, x + 1, y + 1], 1)


def _case(name, table, iou, nms=0.5, capacity=None, **thresholds):
    t = dict(PASS, **thresholds)
    return dict(id=name, table=np.ascontiguousarray(table, np.int32), iou=np.asarray(iou, F), nms_iou_thresh=nms,
                capacity=capacity if capacity is not None else len(table) + 3, **t)


def _mixed(n, seed):
    """random boxes in a 256^2 plane, iou predictions on a coarse lattice (many ties), a few failing each filter, a few NaN"""
    rng = np.random.default_rng(seed)
    x0, y0 = rng.integers(0, 200, n), rng.integers(0, 200, n)
    w, h = rng.integers(0, 56, n), rng.integers(0, 56, n)  # 0: degenerate
    boxes = np.stack([x0, y0, x0 + w, y0 + h], 1)
    if n > 8:  # clusters: near-copies of earlier boxes, so that NMS has work
        src = rng.integers(0, n // 2, n // 3)
        boxes[n - len(src):] = boxes[src] + rng.integers(-2, 3, (len(src), 4))
        boxes[:, 2:] = np.maximum(boxes[:, 2:], boxes[:, :2])
    iou = (rng.integers(0, 24, n) / 24).astype(F) + F(0.25)
    t = _table(boxes)
    t[:, 1] = rng.integers(0, 5, n) * 100          # uni 0 fails
    t[:, 0] = (t[:, 1] * rng.choice([0.25, 0.5, 0.75, 1.0], n)).astype(np.int32)  # inter = exactly thresh * uni passes
    if n > 4:
        iou[rng.integers(0, n, max(1, n // 16))] = np.nan
    return t, iou


def rank_nms_cases():
    cases = []
    for n in (1, 2, 63, 64, 65, 130, 4097):
        t, iou = _mixed(n, n)
        cases.append(_case(f"mixed-{n}", t, iou, nms=0.3137))
        cases.append(_case(f"mixed-{n}-cut", t, iou, nms=0.6181, capacity=max(1, n // 7)))
    for n in (2, 65, 130):
        cases.append(_case(f"disjoint-{n}", _table(_disjoint(n)), np.linspace(0.6, 0.9, n)))
        cases.append(_case(f"identical-{n}", _table(np.tile([10, 20, 50, 90], (n, 1))), np.linspace(0.9, 0.6, n)))
        cases.append(_case(f"equal-scores-{n}", _table(np.tile([[0, 0, 9, 9], [100, 100, 120, 130]], (n, 1))[:n]), np.full(n, 0.75)))
    cases.append(_case("identical-4097", _table(np.tile([0, 0, 255, 255], (4097, 1))), np.full(4097, 0.9)))
    # a chain: B falls to A, so C (which only B would suppress) survives; ranked A, B, C by their scores, stored out of order
    cases.append(_case("chain", _table([[20, 0, 40, 10], [0, 0, 20, 10], [10, 0, 30, 10]]), [0.7, 0.9, 0.8], nms=0.3137))
    # an IoU exactly at the threshold: inter 2, union 4, thresh 0.5 -> not suppressed; one pixel more overlap -> suppressed
    cases.append(_case("iou-at-threshold", _table([[0, 0, 1, 3], [0, 1, 1, 4]]), [0.9, 0.8], nms=0.5))
    cases.append(_case("iou-above-threshold", _table([[0, 0, 1, 4], [0, 1, 1, 4]]), [0.9, 0.8], nms=0.5))
    cases.append(_case("degenerate", _table([[5, 5, 5, 5], [5, 5, 5, 5], [0, 0, 0, 9], [0, 0, 0, 9], [3, 3, 9, 3], [0, 0, 0, 0]]), [0.9, 0.8, 0.7, 0.95, 0.6, 0.65], nms=0.0))
    t, iou = _mixed(70, 7)
    cases.append(_case("all-fail-iou", t, iou, pred_iou_thresh=5.0))
    cases.append(_case("all-fail-stability", t, iou, stability_thresh=1.5))
    cases.append(_case("all-nan", _table(_disjoint(5)), np.full(5, np.nan)))
    cases.append(_case("nan-and-inf", _table(_disjoint(6)), [np.nan, 0.9, np.inf, -np.inf, 0.9, np.nan]))
    cases.append(_case("capacity-1", _table(_disjoint(130)), np.linspace(0.6, 0.9, 130), capacity=1))
    cases.append(_case("disjoint-16384", _table(_disjoint(16384)), 0.6 + (np.arange(16384) % 4099) / 16384, capacity=300))
    return cases


RANK_NMS_CASES = rank_nms_cases()


def score_planes(mask_size, P, n_stored=4, seed=0):
    """f16 [P][n_stored][M][M]: smooth blobs plus noise, then per (prompt, plane) one of the special planes in turn"""
    rng = np.random.default_rng(seed + mask_size)
    M = mask_size
    yy, xx = np.meshgrid(np.linspace(-3, 3, M), np.linspace(-3, 3, M), indexing="ij")
    base = 2.5 * np.sin(2 * xx) * np.cos(3 * yy) - 1.0
    planes = np.empty((P, n_stored, M, M), np.float16)
    for p in range(P):
        for c in range(n_stored):
            planes[p, c] = (np.roll(base, (3 * p + c, 5 * c + p), (0, 1)) + 0.6 * rng.standard_normal((M, M), np.float32)).astype(np.float16)
    return planes


def special_planes(mask_size, cw, ch, off):
    """{name: f16 [M][M]} the planes the kernel must get exactly right, for a region cw x ch and offset `off`"""
    M = mask_size
    out = {}
    out["all-below"] = np.full((M, M), -off - 1.0, np.float16)
    out["all-above"] = np.full((M, M), off + 1.0, np.float16)
    corners = np.full((M, M), -off - 2.0, np.float16)
    for (x, y) in ((0, 0), (cw - 1, 0), (0, ch - 1), (cw - 1, ch - 1)):
        corners[y, x] = off + 3.0
    if cw < M:
        corners[ch // 2, cw] = off + 3.0   # just outside: must not count
    if ch < M:
        corners[ch, cw // 2] = off + 3.0
    out["corners"] = corners
    inner = np.full((M, M), -off - 2.0, np.float16)
    inner[ch // 2, cw // 2] = 0.5 if off >= 0.5 else off + 1
    out["one-pixel"] = inner
    exact = np.empty((M, M), np.float16)
    exact[...] = np.array([off, -off, 0.0, -0.0], np.float16)[(np.arange(M)[:, None] + np.arange(M)[None, :]) % 4]  # exactly at the three comparisons
    out["exactly-at"] = exact
    inf = np.where((np.arange(M)[:, None] + np.arange(M)[None, :]) % 3 == 0, np.inf, -np.inf).astype(np.float16)
    out["inf"] = inf
    out["outside-only"] = np.full((M, M), -off - 2.0, np.float16)
    if cw < M:
        out["outside-only"][:, cw:] = off + 5.0
    if ch < M:
        out["outside-only"][ch:, :] = off + 5.0
    return out

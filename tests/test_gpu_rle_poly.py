"""kernels_rle_poly.hip against tests/rle_poly_ref.py, by equality on whole guarded buffers (tests/buffer_check.py): vx_poly_rle in its three forms on the smallest
polygons that can break a stage, vx_bits_merge and vx_rle_bbox against numpy on decoded reference masks, and the Python entries end to end."""
from functools import lru_cache

import numpy as np
import pytest

from tests import buffer_check as BC
from tests import gpu_util as G
from tests import rle_decode_ref as DR
from tests import rle_poly_ref as ref
from tests.test_rle_poly_ref_cpu import random_polygons
from visioncpp_amd import _lib as L

pytestmark = pytest.mark.gpu

FILL, GUARD, UNSET = 0x7A7A7A, 64, -7
EXTENTS = [(1, 1), (1, 7), (7, 1), (30, 20), (65, 63)]
OCTANTS = [(2, 1), (1, 2), (-1, 2), (-2, 1), (-2, -1), (-1, -2), (1, -2), (2, -1)]  # one edge in each, closed
_release_buffers = G.release_fixture()


def zigzag(k, w, h):
    """k vertices from side to side, stepping down: k - 1 edges of 5 w points and w boundary keys each"""
    return [(0.0 if j % 2 == 0 else float(w), (j + 0.5) * h / k) for j in range(k)]


@lru_cache(maxsize=None)
def cases(w, h):
    """-> (polygons, their reference records): named shapes scaled to the extent, then seeded random ones"""
    star, at = [], np.array([0.45 * w, 0.05 * h])
    for d in OCTANTS:
        star.append((float(at[0]), float(at[1])))
        at = at + np.array(d) * (0.17 * w, 0.17 * h)
    named = [[(0.3 * w, 0.4 * h)], [(0.2 * w, 0.1 * h), (0.9 * w, 0.8 * h)], [(0.1 * w, 0.1 * h), (0.1 * w, 0.9 * h), (0.8 * w, 0.6 * h)],
             [(2.0, 2.0), (2.0, 2.0), (w - 1.0, h - 1.0), (w - 1.0, h - 1.0), (2.0, h - 1.0)], star, [(1.0, 1.0), (1.0, h - 1.0), (w - 1.0, h - 1.0), (w - 1.0, 1.0)],
             [(-3.7, -2.2), (w / 2, h + 3.3), (w + 4.6, -1.9)], [(-5.0, -5.0), (-5.0, -1.0), (-1.0, -1.0)], [(0.0, 0.0), (0.0, float(h)), (float(w), float(h)), (float(w), 0.0)],
             [(-2.0, 0.3 * h), (w + 2.0, 0.3 * h), (w + 2.0, h + 2.0), (-2.0, h + 2.0)]]
    polygons = named + random_polygons(w * 100 + h, 30, w, h)
    return polygons, [ref.runs(p, w, h) for p in polygons]


@lru_cache(maxsize=None)
def zigzag_cases(w=64, h=48):
    polygons = [zigzag(20, w, h), zigzag(300, w, h), [(3.0, 4.0), (3.0, 11.0), (12.0, 11.0), (12.0, 4.0)]]
    return polygons, [ref.runs(p, w, h) for p in polygons]


def poly_rle(polygons, w, h, counts=None, base=0):
    """the three forms of vx_poly_rle -> (mk i64 [n, 2], sizes, status, the rows' buffer before, after): rows `base` entries into a buffer of FILL with a guard"""
    from visioncpp_amd import vision
    api, n = G.api(), len(polygons)
    live = n if counts is None else counts
    xy, poff = vision._polygon_rows(polygons)
    tv = int(poff[-1])
    xd, pd = G.dev(xy), G.dev(poff)
    cd = G.dev(np.array([counts, 12345], np.int32)).ptr if counts is not None else None
    mkd, sd, td = G.dev(np.full((n, 2), UNSET, np.int64)), G.dev(np.full(n, UNSET, np.int32)), G.dev(np.full(n, UNSET, np.int32))
    ws = api.vx_poly_rle_workspace_bytes(tv, n, 0)
    L.vx_check(api.vx_poly_rle(xd.ptr, pd.ptr, tv, 0, n, w, h, cd, 0, None, 0, None, None, None, mkd.ptr, td.ptr, G.empty(ws).ptr, ws, None))
    mk = mkd.to_numpy(np.int64, (n, 2))
    longest, total_keys = int(mk[:live, 0].max()), sum(api.vx_poly_rle_key_row(int(k)) for k in mk[:live, 1])
    ws = api.vx_poly_rle_workspace_bytes(tv, n, longest)
    wd, kd = G.empty(ws), G.empty(4 * total_keys + 16)
    L.vx_check(api.vx_poly_rle(xd.ptr, pd.ptr, tv, longest, n, w, h, cd, 0, kd.ptr, total_keys, None, None, sd.ptr, None, td.ptr, wd.ptr, ws, None))
    sizes = sd.to_numpy(np.int32, (n,))
    offsets = np.concatenate([[0], np.cumsum(np.where(np.arange(n) < live, sizes, 0))]).astype(np.int64)
    before = np.full(base + int(offsets[-1]) + GUARD, FILL, np.uint32)
    rd = G.dev(before)
    L.vx_check(api.vx_poly_rle(xd.ptr, pd.ptr, tv, longest, n, w, h, cd, 0, kd.ptr, total_keys, rd.ptr + 4 * base, G.dev(offsets).ptr, None, None, td.ptr, wd.ptr, ws, None))
    G.sync()
    return mk, sizes, td.to_numpy(np.int32, (n,)), before, rd.to_numpy(np.uint32, before.shape)


def assert_rows(run, want, skipped, base, what):
    """the rows of `want` one behind the other from `base` on, every other entry as it was; sizes and status of skipped polygons untouched"""
    mk, sizes, status, before, got = run
    flat = np.array([c for r in want for c in r], np.float64)
    expect, written = before.astype(np.float64), np.zeros(before.shape, bool)
    expect[base:base + len(flat)] = flat
    written[base:base + len(flat)] = True
    BC.assert_buffer(got.astype(np.float64), (expect, np.zeros(before.shape), written), what, untouched=before.astype(np.float64))
    assert sizes.tolist() == [len(r) for r in want] + [UNSET] * skipped and status.tolist() == [0] * len(want) + [UNSET] * skipped, what


@pytest.mark.parametrize("w, h", EXTENTS, ids=[f"{w}x{h}" for w, h in EXTENTS])
def test_polygons_equal_the_reference(w, h):
    polygons, want = cases(w, h)
    run = poly_rle(polygons, w, h, base=3)
    assert run[0].tolist() == [[len(ref.points(p)[0]), len(ref.keys(p, w, h)) + 1] for p in polygons]  # the count pass alone
    assert_rows(run, want, 0, 3, f"polygons {w}x{h}")
    assert want[7] == [w * h] and want[8][0] == 0 and all(sum(r) == w * h for r in want)  # wholly outside; covering pixel 0
    assert poly_rle(polygons, w, h, base=3)[4].tobytes() == run[4].tobytes(), "the second call gave other bytes"
    assert_rows(poly_rle(polygons, w, h, counts=3), want[:3], len(polygons) - 3, 0, f"polygons {w}x{h} with a device count of 3")


def test_long_outlines_cross_a_point_chunk_and_the_lds_sort(w=64, h=48):
    polygons, want = zigzag_cases()
    run = poly_rle(polygons, w, h)
    assert 4096 < run[0][0, 0] and run[0][0, 1] <= 8192 < run[0][1, 1]  # more than one chunk of points; keys sorted in LDS and in global memory
    assert_rows(run, want, 0, 0, "zigzags 64x48")


def test_a_refused_polygon_has_a_status_and_no_row(w=30, h=20):
    from visioncpp_amd import vision
    polygons, want = cases(w, h)
    rows = [polygons[2], [(1.0, float("nan")), (4.0, 5.0)], polygons[4], [(2.0 ** 20 + 1, 0.0)], polygons[5]]
    api, (xy, poff) = G.api(), vision._polygon_rows(rows)
    poff = np.concatenate([poff, poff[-1:]])  # a sixth polygon without vertices
    xd, pd, n = G.dev(xy), G.dev(poff), 6
    mkd, sd, td = G.dev(np.zeros((n, 2), np.int64)), G.dev(np.full(n, UNSET, np.int32)), G.dev(np.full(n, UNSET, np.int32))
    ws = api.vx_poly_rle_workspace_bytes(int(poff[-1]), n, 0)
    wd, kd = G.empty(ws), G.empty(4 * 4096)
    L.vx_check(api.vx_poly_rle(xd.ptr, pd.ptr, int(poff[-1]), 0, n, w, h, None, 0, None, 0, None, None, None, mkd.ptr, td.ptr, wd.ptr, ws, None))
    L.vx_check(api.vx_poly_rle(xd.ptr, pd.ptr, int(poff[-1]), 0, n, w, h, None, 0, kd.ptr, 4096, None, None, sd.ptr, None, td.ptr, wd.ptr, ws, None))
    G.sync()
    good = [want[2], want[4], want[5]]
    assert td.to_numpy(np.int32, (n,)).tolist() == [0, 2, 0, 2, 0, 1] and sd.to_numpy(np.int32, (n,)).tolist() == [len(good[0]), 0, len(good[1]), 0, len(good[2]), 0]
    assert mkd.to_numpy(np.int64, (n, 2))[[1, 3, 5]].tolist() == [[0, 0]] * 3


def bit_words(masks, w, h):
    """bool [n, h, w] -> u64 [n, w * S]: word (x, s) at x * S + s, bit r row 64 s + r"""
    S = (h + 63) // 64
    padded = np.zeros((len(masks), S * 64, w), np.uint8)
    padded[:, :h] = masks
    return np.packbits(padded.transpose(0, 2, 1), axis=-1, bitorder="little").reshape(len(masks), w * S * 8).view(np.uint64)


@pytest.mark.parametrize("intersect", [0, 1], ids=["or", "and"])
@pytest.mark.parametrize("w, h", [(65, 63), (20, 130)])
def test_bits_merge_equals_numpy(w, h, intersect):
    api = G.api()
    polygons, rows = cases(w, h)
    rows = [rows[i] for i in (5, 9, 4, 2, 6, 8)]  # groups of 0, 1 and 5 members
    masks = np.stack([DR.decode(r, w, h)[0] for r in rows])
    fold = np.bitwise_and.reduce if intersect else np.bitwise_or.reduce
    want = np.stack([np.zeros((h, w), bool), masks[0], fold(masks[1:6])])
    assert len({m.tobytes() for m in masks}) == 6 and (intersect or want[2].any())
    (offsets, runs), per = DR.csr(rows), api.vx_mask_rle_workspace_bytes(w, h, 1) // 8
    wd, ws = G.empty(6 * per * 8), api.vx_rle_to_bits_workspace_bytes(len(runs), 6)
    L.vx_check(api.vx_rle_to_bits(G.dev(runs).ptr, G.dev(offsets).ptr, len(runs), 6, w, h, None, 0, wd.ptr, None, None, G.empty(ws).ptr, ws, None))
    fill = np.full((3, per), 0x5A5A5A5A5A5A5A5A, np.uint64)
    out = G.dev(fill)
    L.vx_check(api.vx_bits_merge(wd.ptr, 6, G.dev(np.array([0, 0, 1, 6], np.int64)).ptr, 3, w, h, intersect, out.ptr, None))
    G.sync()
    expect = fill.copy()
    expect[:, :w * ((h + 63) // 64)] = bit_words(want, w, h)
    assert np.array_equal(out.to_numpy(np.uint64, fill.shape), expect)


@pytest.mark.parametrize("w, h", [(30, 20), (65, 63), (1, 1)])
def test_boxes_equal_numpy(w, h):
    api = G.api()
    rows = cases(w, h)[1] + [[w * h], [max(h - 2, 0), min(5, w * h - max(h - 2, 0)), w * h], [0, 1], [w * h // 2, 3 * w * h], list(range(1, 40)) * 30, [1]]
    (offsets, runs), n = DR.csr(rows), len(rows)
    want = np.full((n + 4, 4), UNSET, np.int64)
    want[:n - 1] = [ref.box(DR.decode(r, w, h)[0]) for r in rows[:-1]]  # a device count keeps the last row out
    out = G.dev(np.full((n + 4, 4), UNSET, np.int32))
    L.vx_check(api.vx_rle_bbox(G.dev(runs).ptr, G.dev(offsets).ptr, len(runs), n, w, h, G.dev(np.array([n - 1], np.int32)).ptr, 0, out.ptr, None))
    G.sync()
    assert np.array_equal(out.to_numpy(np.int32, (n + 4, 4)), want)
    assert want[len(cases(w, h)[1])].tolist() == [0, 0, 0, 0]  # the empty mask


def test_python_entries_end_to_end(w=65, h=63):
    from visioncpp_amd import vision
    polygons, rows = cases(w, h)
    flat = [[c for xy in polygons[i] for c in xy] for i in (2, 4)]
    both = DR.decode(rows[2], w, h)[0] | DR.decode(rows[4], w, h)[0]
    got = vision.fr_py_objects([flat, flat[:1]], h, w)
    assert [r["size"] for r in got] == [[h, w]] * 2 and np.array_equal(vision.rle_decode(got), np.stack([both, DR.decode(rows[2], w, h)[0]]))
    assert vision.fr_py_objects(got[0], h, w) is got[0] and vision.poly_to_rle(polygons[:12], h, w) == [{"size": [h, w], "counts": r} for r in rows[:12]]
    boxes = np.array([[3, 4, 9, 7], [0, 0, w, h], [w - 1, h - 1, 1, 1], [10, 0, 1, h]], np.int32)
    records = vision.fr_py_objects(boxes.tolist(), h, w)
    want = np.zeros((4, h, w), np.uint8)
    for m, (x, y, bw, bh) in zip(want, boxes):
        m[y:y + bh, x:x + bw] = 1
    assert np.array_equal(vision.rle_decode(records), want) and np.array_equal(vision.rle_to_bbox(vision.bbox_to_rle(boxes, h, w)), boxes)
    assert np.array_equal(vision.rle_decode(vision.rle_merge(records[:2] + records[3:], intersect=True)), want[0] & want[1] & want[3])

"""tests/rle_poly_ref.py against itself (the loop's step 4 against the odd-group rule), against a vector that can be drawn by hand and against the host
restatement in csrc/mask_rle.cpp, and what the polygon entries refuse before anything touches a device. No GPU."""
import ctypes as C

import numpy as np
import pytest

from tests import rle_decode_ref as DR
from tests import rle_poly_ref as ref
from visioncpp_amd import _lib as L
from visioncpp_amd import vision

_buf = C.create_string_buffer(4096)
P = (C.addressof(_buf) + 15) & ~15  # 16-byte aligned zeros, never written: every call below is refused first
RECT = [(3, 4), (3, 11), (12, 11), (12, 4)]


def random_polygons(seed, count, w, h):
    """1 .. 8 vertices inside and outside the extent, one polygon in three with integer vertices"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(count):
        p = rng.uniform((-0.4 * w, -0.4 * h), (1.4 * w, 1.4 * h), (int(rng.integers(1, 9)), 2))
        out.append([(float(x), float(y)) for x, y in (np.rint(p) if i % 3 == 0 else p)])
    return out


def host_restatement(polygons, w, h):
    xy, poff = vision._polygon_rows(polygons)
    offsets, runs, owner = np.zeros(len(poff), np.int64), C.c_void_p(), C.c_void_p()
    L.check(L.get_lib().visp_image_rle_from_poly_reference_host(xy.ctypes.data, poff.ctypes.data, len(polygons), w, h, offsets.ctypes.data, C.byref(runs), C.byref(owner)))
    return [r["counts"] for r in vision._rle_records(offsets, runs, owner, len(polygons), w, h)]


def test_step_four_is_the_odd_group_rule_and_records_sum_to_the_extent(w=30, h=20):
    polygons = random_polygons(3, 600, w, h)
    want = [ref.runs(p, w, h) for p in polygons]
    assert all(sum(r) == w * h for r in want) and want == [ref.runs_by_parity(p, w, h) for p in polygons]
    assert sum(len(k) != len(set(k)) for k in (ref.keys(p, w, h) for p in polygons[::3])) > 50  # integer vertices do give cancelling pairs
    assert host_restatement(polygons, w, h) == want


def test_the_rectangle_decodes_to_its_pixels(w=30, h=20):
    want = np.zeros((h, w), bool)
    want[4:11, 3:12] = True
    assert np.array_equal(DR.decode(ref.runs(RECT, w, h), w, h)[0], want) and ref.box(want) == [3, 4, 9, 7]
    assert ref.runs([(-5.0, -5.0), (-5.0, -1.0), (-1.0, -1.0)], w, h) == [w * h] and ref.runs(ref.box_polygon((0, 0, 2, 1)), w, h)[0] == 0


BAD = [("nan", [[(1.0, 2.0)], [(1.0, float("nan")), (2.0, 3.0)]], 30, 20, "polygon 1, vertex 0"), ("inf", [[(float("inf"), 2.0)]], 30, 20, "polygon 0, vertex 0"),
       ("beyond", [RECT, RECT, [(0.0, 0.0), (2.0 ** 20 + 1, 0.0)]], 30, 20, "polygon 2, vertex 1"), ("no vertex", [RECT, []], 30, 20, "polygon 1 has no vertex"),
       ("extent", [RECT], 65536, 32768, "extent 65536x32768")]


@pytest.mark.parametrize("polygons, w, h, message", [c[1:] for c in BAD], ids=[c[0] for c in BAD])
def test_host_entries_refuse_bad_polygons_before_any_device_call(polygons, w, h, message):
    with pytest.raises(L.Error, match=f"rle_from_poly: {message}"):
        vision.poly_to_rle(polygons, h, w)


def test_entries_refuse_bad_arguments_before_any_device_call():
    api = L.get_lib()
    xy, down = np.arange(12, dtype=np.float64), np.array([0, 4, 2], np.int64)
    with pytest.raises(L.Error, match="rle_from_poly: offsets decrease at polygon 1"):
        L.check(api.visp_image_rle_from_poly_host(xy.ctypes.data, down.ctypes.data, 2, 30, 20, P, P, P, None))
    for fn, args in [("from_poly_host", (None, P, 1, 8, 8, P, P, P, None)), ("from_poly_host", (P, P, 0, 8, 8, P, P, P, None)), ("from_poly_host", (P, P, 1, 8, 8, P, None, P, None)),
                     ("from_poly_device", (None, P, 1, 8, 8, None, None, None, P, None, None, None)), ("from_poly_device", (P, P, 1, 8, 8, None, P, None, None, None, None, None)),
                     ("from_poly_device", (P, P, 70000, 8, 8, None, None, None, P, None, None, None)), ("from_bbox_host", (None, 1, 8, 8, P, P, P, None)),
                     ("from_bbox_host", (P, 1, 0, 8, P, P, P, None)), ("merge_host", (P, P, 1, None, 1, 8, 8, 0, P, P, P, None)), ("merge_host", (P, P, 1, P, 0, 8, 8, 0, P, P, P, None)),
                     ("merge_device", (P, P, 1, P, 1, 8, 8, 0, 0, P, None, None)), ("merge_device", (P, None, 1, P, 1, 8, 8, 0, 1, P, None, None)),
                     ("to_bbox_host", (P, P, 1, 8, 8, None, None)), ("to_bbox_device", (P, P, 0, 8, 8, None, P, None, None))]:
        with pytest.raises(L.Error, match="rle_(from_poly|from_bbox|merge|to_bbox)"):
            L.check(getattr(api, f"visp_image_rle_{fn}")(*args))
    groups = np.array([0, 2], np.int64)  # two records asked of one
    with pytest.raises(L.Error, match="rle_merge: group 0 is records 0 .. 2 of 1"):
        L.check(api.visp_image_rle_merge_host(np.array([0, 1], np.int64).ctypes.data, np.array([64], np.uint32).ctypes.data, 1, groups.ctypes.data, 1, 8, 8, 0, P, P, P, None))
    assert api.vx_poly_rle_workspace_bytes(0, 1, 0) == 0 and api.vx_poly_rle_workspace_bytes(10, 70000, 0) == 0 and api.vx_poly_rle_workspace_bytes(10, 2, 0) % 256 == 0
    assert [api.vx_poly_rle_key_row(k) for k in (1, 8192, 8193, 20000)] == [1, 8192, 16384, 32768]
    for call in (lambda: api.vx_poly_rle(P, P, 4, 0, 1, 8, 8, None, 0, None, 0, None, None, None, None, None, P, 4096, None),
                 lambda: api.vx_poly_rle(P, P, 4, 0, 1, 8, 8, None, 0, P, 64, None, None, None, None, None, P, 4096, None),
                 lambda: api.vx_poly_rle(P, P, 4, 0, 1, 8, 0, None, 0, None, 0, None, None, None, P, None, P, 4096, None),
                 lambda: api.vx_poly_rle(P, P, 4, 0, 1, 8, 8, None, 0, None, 0, None, None, None, P, None, P, 16, None),
                 lambda: api.vx_bits_merge(P, 1, None, 1, 8, 8, 0, P, None), lambda: api.vx_bits_merge(P, 1, P, 0, 8, 8, 0, P, None),
                 lambda: api.vx_rle_bbox(P, P, 0, 1, 8, 8, None, 0, None, None), lambda: api.vx_rle_bbox(P, P, 0, 0, 8, 8, None, 0, P, None)):
        assert call() == 0 and b"vx_" in api.vx_last_error()

"""tests/rle_decode_ref.py against the encoder's definition (tests/rle_ref.py) and a direct IoU, and what the decode / area / IoU entries refuse before anything
touches a device. These run without a GPU."""
import ctypes as C

import numpy as np
import pytest

from tests import rle_cases as RC
from tests import rle_decode_ref as DR
from tests import rle_ref as RR
from visioncpp_amd import _lib as L
from visioncpp_amd import vision

_buf = C.create_string_buffer(4096)
P = (C.addressof(_buf) + 15) & ~15  # 16-byte aligned zeros: offsets {0, 0, ..}, never written: every call below is refused first


@pytest.mark.parametrize("w, h", [(37, 53), (64, 64), (1, 70)])
def test_reference_inverts_the_encoder_and_equals_a_direct_iou(w, h):
    masks = np.stack(list(RC.named_masks(w, h).values())) != 0
    for m in masks:
        got, area, status = DR.decode(RR.mask_to_rle(m)["counts"], w, h)
        assert np.array_equal(got, m) and area == m.sum() and status == 0
    inter, den, iou = DR.iou(masks, masks[::-1])
    for i, a in enumerate(masks):
        for j, b in enumerate(masks[::-1]):
            union = int((a | b).sum())
            assert inter[i, j] == (a & b).sum() and den[i, j] == union and iou[i, j] == ((a & b).sum() / union if union else 0.0)
    assert np.array_equal(DR.iou(masks, masks, np.ones(8, bool))[1], np.repeat(masks.sum((1, 2))[:, None], 8, 1))  # crowd: a's area


def test_reference_clamps_short_and_long_rows():
    short, area, status = DR.decode([3, 4], 4, 4)
    assert (status, area) == (1, 4) and short.T.ravel().tolist() == [False] * 3 + [True] * 4 + [False] * 9
    long_, area, status = DR.decode([10, 9, 5, 5], 4, 4)
    assert (status, area) == (2, 6) and long_.T.ravel().tolist() == [False] * 10 + [True] * 6


def test_decode_and_area_entries_refuse_before_any_device_call():
    api = L.get_lib()
    offsets, runs = DR.csr([[3, 4, 57], [10, 50]])  # 8 x 8: row 1 sums to 60
    o, r = offsets.ctypes.data, runs.ctypes.data
    for args, msg in [((None, r, 2, 8, 8, 1, P, None), "null"), ((o, None, 2, 8, 8, 1, P, None), "null"), ((o, r, 2, 8, 8, 1, None, None), "null"),
                      ((o, r, 0, 8, 8, 1, P, None), "0 masks"), ((o, r, 1, 65536, 32768, 1, P, None), "extent"), ((o, r, 1, 8, 0, 1, P, None), "extent"),
                      ((o, r, 1, 8, 8, 256, P, None), "value"), ((o, r, 2, 8, 8, 1, P, None), "row 1 sum to 60")]:
        with pytest.raises(L.Error, match=f"rle_decode.*{msg}"):
            L.check(api.visp_image_rle_decode_host(*args))
    for args in ((None, P, 1, 8, 8, None, 1, P, None, None, None, None), (P, P, 1, 8, 8, None, 1, None, None, None, None, None), (P, P, 1, 8, 8, None, 0, P, None, None, None, None),
                 (P, P, 70000, 8, 8, None, 1, P, None, None, None, None), (P, P, 1, 1, 2 ** 31 - 1, None, 1, P, None, None, None, None)):
        with pytest.raises(L.Error, match="rle_decode"):
            L.check(api.visp_image_rle_decode_device(*args))
    with pytest.raises(L.Error, match="rle_area.*null"):
        L.check(api.visp_image_rle_area_host(o, r, 2, None))
    with pytest.raises(ValueError, match="differ in size"):
        vision.rle_decode([{"size": [8, 8], "counts": [64]}, {"size": [8, 9], "counts": [72]}])
    assert vision.rle_area([{"size": [8, 8], "counts": [3, 4, 57]}, {"size": [8, 8], "counts": [0, 64]}]).tolist() == [4, 64]  # host code


def test_iou_entries_refuse_before_any_device_call():
    api = L.get_lib()
    offsets, runs = DR.csr([[3, 4, 57], [10, 50]])
    o, r = offsets.ctypes.data, runs.ctypes.data
    rle8, masks8, masks9 = (None, r, o, 1, 8, 8), (P, None, None, 1, 8, 8), (P, None, None, 1, 8, 9)
    for a, b, out, msg in [(rle8, masks9, P, "extents differ, 8x8 and 8x9"), (rle8, (None, None, None, 1, 8, 8), P, "null"), ((P, r, o, 1, 8, 8), masks8, P, "both forms"),
                           (rle8, masks8, None, "null"), (masks8, (None, r, o, 2, 8, 8), P, "row 1 sum to 60"), ((P, None, None, 0, 8, 8), masks8, P, "0 masks")]:
        with pytest.raises(L.Error, match=f"mask_iou.*{msg}"):
            L.check(api.visp_image_mask_iou_host(*a, *b, None, out, None, None))
    with pytest.raises(L.Error, match="mask_iou.*extents differ"):
        L.check(api.visp_image_mask_iou_device(*masks8, *masks9, None, P, None, None, None))
    assert api.vx_rle_to_bits_workspace_bytes(100, 3) == 512 and api.vx_rle_to_bits_workspace_bytes(-1, 3) == 0 and api.vx_bitmask_iou_workspace_bytes(8, 8) == 256
    for call in (lambda: api.vx_rle_to_bits(P, P, 0, 1, 0, 8, None, 0, P, None, None, P, 4096, None), lambda: api.vx_bits_to_mask_u8(P, 1, 8, 8, None, 0, 0, P, None),
                 lambda: api.vx_mask_to_bits_u8(P, 1, 8, 8, None, 0, P + 4, None), lambda: api.vx_bitmask_iou(P, 1, P, 1, 8, 8, None, None, None, None, P, P, 8, None)):
        assert call() == 0 and b"vx_" in api.vx_last_error()

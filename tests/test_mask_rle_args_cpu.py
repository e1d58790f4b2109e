"""What the RLE launcher and C entries refuse, they refuse before anything touches a device; rle_to_mask is host code. These run without a GPU."""
import ctypes as C

import numpy as np
import pytest

from tests import rle_cases as RC
from tests import rle_ref as RR
from visioncpp_amd import _lib as L
from visioncpp_amd import vision

_buf = C.create_string_buffer(128)
P = (C.addressof(_buf) + 15) & ~15  # 16-byte aligned, never read: every call below is refused first
GOOD = dict(masks=P, w=8, h=8, n=2, counts=None, runs=P, run_stride=65, n_runs=P, workspace=P, workspace_bytes=1 << 20, group=2, stream=None)
BAD = [dict(masks=None), dict(n_runs=None), dict(workspace=None), dict(w=0), dict(h=0), dict(w=65536, h=32768), dict(w=1, h=2 ** 31 - 1), dict(n=0), dict(group=0), dict(run_stride=-1),
       dict(workspace_bytes=511), dict(workspace=P + 8)]


@pytest.mark.parametrize("change", BAD, ids=[f"{k}-{i}" for i, c in enumerate(BAD) for k in list(c)[:1]])
def test_launcher_refuses_before_any_device_call(change):
    api = L.get_lib()
    assert api.vx_mask_rle_u8(*{**GOOD, **change}.values()) == 0 and b"vx_mask_rle_u8" in api.vx_last_error(), api.vx_last_error()


def test_packed_launcher_refuses_before_any_device_call():
    api = L.get_lib()
    for args in ((P, 8, 8, 2, None, P, P, P, 1 << 20, 2, None), (P, 8, 8, 2, P, None, P, P, 1 << 20, 2, None), (P, 0, 8, 2, P, P, P, P, 1 << 20, 2, None)):
        assert api.vx_mask_rle_packed_u8(*args) == 0 and b"vx_mask_rle_packed_u8" in api.vx_last_error(), api.vx_last_error()


def test_workspace_is_one_bit_per_pixel_in_whole_column_words(ws=L.get_lib().vx_mask_rle_workspace_bytes):
    assert ws(8, 8, 2) == 2 * 256 and ws(1024, 1024, 1) == 1024 * 16 * 8 and ws(64, 65, 1) == 64 * 2 * 8
    assert ws(0, 8, 1) == 0 and ws(8, 8, 0) == 0 and ws(65536, 32768, 1) == 0


def test_c_entries_refuse_before_any_device_call():
    api = L.get_lib()
    for args in ((None, 1, 8, 8, None, P, 65, P, None, None), (P, 0, 8, 8, None, P, 65, P, None, None), (P, 1, 0, 8, None, P, 65, P, None, None),
                 (P, 1, 65536, 32768, None, P, 65, P, None, None), (P, 1, 8, 8, None, P, -1, P, None, None), (P, 1, 8, 8, None, P, 65, None, None, None)):
        with pytest.raises(L.Error, match="rle_encode"):
            L.check(api.visp_image_rle_encode_device(*args))
    for args in ((None, 1, 8, 8, P, P, P, None), (P, 0, 8, 8, P, P, P, None), (P, 1, 8, 0, P, P, P, None), (P, 1, 8, 8, None, P, P, None)):
        with pytest.raises(L.Error, match="rle_encode"):
            L.check(api.visp_image_rle_encode_host(*args))
    with pytest.raises(L.Error, match="null argument"):  # refused before the handle is looked at
        L.check(api.visp_sam_generate_masks_rle_host(None, P, P, 1, 0.5, 0.5, 1.0, 0.7, 4, 0, P, P, P, P, None, P))
    with pytest.raises(L.Error, match="capacity"):
        L.check(api.visp_sam_generate_masks_rle_host(None, P, P, 1, 0.5, 0.5, 1.0, 0.7, 0, 0, P, P, P, P, P, P))


def test_unknown_output_mode():
    with pytest.raises(ValueError, match="binary_mask.*uncompressed_rle"):
        vision.Model.sam_generate_masks(None, output_mode="coco_rle")


@pytest.mark.parametrize("name", ["first", "edges", "random"])
def test_rle_to_mask_inverts_the_reference(name):
    m = RC.named_masks(65, 63)[name]
    assert np.array_equal(vision.rle_to_mask(RR.mask_to_rle(m)), m != 0)

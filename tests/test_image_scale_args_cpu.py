"""What the device image_scale entries refuse, they refuse with a message of their own before anything touches a device: these run without a GPU,
where a device call would fail with HIP's message instead."""
import ctypes as C

import pytest

from visioncpp_amd import _lib as L

RGB_U8, ALPHA_U8, RGBA_F32 = 3, 4, 5
PTR = C.cast(C.create_string_buffer(64), C.c_void_p)  # never read: every call below is refused first


def _refused(ok, needle: bytes):
    msg = L.get_lib().visp_get_last_error()
    assert ok == 0 and needle in msg, msg


# src, format, batch, w, h, dst, out_w, out_h -> the message
BAD = [pytest.param((None, RGB_U8, 1, 8, 8, PTR, 4, 4), b"null pointer", id="null-src"),
       pytest.param((PTR, RGB_U8, 1, 8, 8, None, 4, 4), b"null pointer", id="null-dst"),
       pytest.param((PTR, 8, 1, 8, 8, PTR, 4, 4), b"Unsupported image format [8]", id="format-8"),
       pytest.param((PTR, -1, 1, 8, 8, PTR, 4, 4), b"Unsupported image format [-1]", id="format-negative"),
       pytest.param((PTR, RGBA_F32, 0, 8, 8, PTR, 4, 4), b"batch 0 must be at least 1", id="batch-0"),
       pytest.param((PTR, RGB_U8, 1, 0, 8, PTR, 4, 4), b"Failed to resize image 0x8 to 4x4", id="source-extent"),
       pytest.param((PTR, RGB_U8, 1, 8, 8, PTR, 4, -2), b"Failed to resize image 8x8 to 4x-2", id="target-extent"),
       pytest.param((PTR, ALPHA_U8, 1, 2000, 4, PTR, 10, 4), b"reducing 2000 to 10 takes 800 taps per output sample, the device kernel holds at most 768", id="ratio-x"),
       pytest.param((PTR, RGBA_F32, 2, 4, 100000, PTR, 4, 1), b"reducing 100000 to 1 takes 400000 taps", id="ratio-y")]


@pytest.mark.parametrize("args, needle", BAD)
def test_scale_entries_refuse_before_any_device_call(args, needle):
    api = L.get_lib()
    src, fmt, batch, w, h, dst, ow, oh = args
    _refused(api.visp_image_scale_batch_device(None, src, fmt, batch, w, h, dst, ow, oh, None), needle)
    _refused(api.visp_image_scale_batch_host(None, src, fmt, batch, w, h, dst, ow, oh), needle)


def test_depthany_scaled_entries_refuse_a_null_model():
    api = L.get_lib()
    _refused(api.visp_depthany_compute_scaled_batch_device(None, PTR, 1, 8, 8, PTR, None), b"model handle is null")
    _refused(api.visp_depthany_compute_scaled_batch_host(None, PTR, 1, 8, 8, PTR), b"model handle is null")


def test_launcher_refuses_null_pointers():
    assert L.get_lib().vx_image_scale(None, RGB_U8, 1, 8, 8, None, 4, 4, None, 0, 64, 4, 4, 8, None) == 0
    assert b"vx_image_scale: null pointer" in L.get_lib().vx_last_error()

"""The matting image ops without a GPU: the float64 restatement (tests/matting_ref.py) meets the reference's own test vectors
(tests/golden/image_ops_vectors.json, from the reference's tests/test-image.cpp:205-281) under the reference's criterion (rms <= 1e-5,
tests/testing.cpp:12; the composite and the erosion exactly); visp_image_set_alpha / visp_image_to_mask run on the built library; and every refusal
of the new C entries and vx_* launchers comes back as an error text before anything touches a device -- this file never needs one."""
import ctypes as C
import json

import numpy as np
import pytest

import matting_ref as R
from visioncpp_amd import _lib as L
from visioncpp_amd import vision as V
from visioncpp_amd.vision import ImageFormat as F


@pytest.fixture(scope="module")
def vectors(golden_dir):
    return json.loads((golden_dir / "image_ops_vectors.json").read_text())


def rms(a, b):
    return float(np.sqrt(np.mean((np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2)))


def test_reference_restatement_meets_the_blur_vector(vectors):
    v = vectors["blur"]
    w, h = v["extent"]
    x = np.array(v["input"], np.float32).reshape(h, w)
    want = np.array(v["expected"], np.float64).reshape(h, w)
    assert rms(R.box_blur(x, v["radius"]), want) <= 1e-5
    assert rms(R.box_blur_running_f32(x, v["radius"]), want) <= 1e-5  # the reference's own order passes its own test


def test_reference_restatement_meets_the_erosion_vector_exactly(vectors):
    v = vectors["erosion"]
    w, h = v["extent"]
    x = np.array(v["input"], np.float32).reshape(h, w)
    want = np.array(v["expected"], np.float32).reshape(h, w)
    assert np.array_equal(R.erosion(x, v["radius"]), want)
    x8 = (x * 255).astype(np.uint8)
    assert np.array_equal(R.erosion(x8, v["radius"]), (want * np.float32(255)).astype(np.uint8))


def test_reference_restatement_meets_the_composite_vector_exactly(vectors):
    v = vectors["alpha_composite"]
    w, h = v["extent"]
    fg = np.array(v["fg_rgba_u8"], np.uint8).reshape(h, w, 4)
    bg = np.array(v["bg_rgb_u8"], np.uint8).reshape(h, w, 3)
    mask = np.array(v["mask_u8"], np.uint8).reshape(h, w)
    want = np.array(v["expected_rgba_u8"], np.uint8).reshape(h, w, 4)
    assert np.array_equal(R.alpha_composite(fg, bg, mask), want)  # 63 and 191, not 64 and 192: the store truncates


def test_running_sum_mode_differs_from_the_definition_behind_a_bright_region():
    """What DESIGN.md section 21 quotes: behind 40 pixels of 1.0, the reference's f32 running sum is off by far more than a window-local sum may be."""
    x = np.full((64, 200), 1e-4, np.float32)
    x[:, :40] = 1.0
    exact = R.box_blur(x, 30)
    running = R.box_blur_running_f32(x, 30)
    rel = np.abs(running - exact)[:, 80:] / exact[:, 80:]
    assert rel.max() > 50 * 4 * 61 * 2.0 ** -24  # documents the effect; the kernels are not held to this mode


def test_estimator_restatement_properties():
    rng = np.random.default_rng(3)
    img = rng.random((16, 12, 3))
    for mask in (np.zeros((16, 12)), np.ones((16, 12))):
        out = R.estimate_foreground(img, mask, 5)
        assert np.array_equal(out[..., 3], mask)
        if mask[0, 0] == 1:  # an opaque mask gives the image back: bf + 1 * (img - bf)
            assert np.abs(out[..., :3] - img).max() < 1e-4


@pytest.mark.parametrize("fmt", ["rgba_u8", "bgra_u8", "argb_u8"])
def test_set_alpha_and_to_mask_on_the_library(fmt):
    rng = np.random.default_rng(11)
    wide = rng.integers(0, 256, (9, 13 + 5, 4), dtype=np.uint8)
    img = wide[:, 2:15]  # a strided view: 13 pixels of rows that hold 18
    alpha_wide = rng.integers(0, 256, (9, 20), dtype=np.uint8)
    alpha = alpha_wide[:, 3:16]
    got = V.image_set_alpha(img, alpha, F[fmt])
    assert np.array_equal(got, R.set_alpha(img, alpha, fmt))
    assert np.array_equal(V.image_to_mask(img, F[fmt]), R.to_mask(img))
    assert np.array_equal(V.image_to_mask(wide[:, 1:8, :3], F.rgb_u8), wide[:, 1:8, 0])
    assert np.array_equal(V.image_to_mask(alpha, F.alpha_u8), alpha)


def _view(a, fmt):
    return V._view_of(a, fmt)


def _refused(name, *args):
    api = L.get_lib()
    out_view, out_data = L.ImageView(), C.c_void_p()
    ok = getattr(api, name)(*args, C.byref(out_view), C.byref(out_data))
    assert ok == 0 and not out_data.value, f"{name} accepted what it must refuse"
    return api.visp_get_last_error().decode()


def test_host_entries_refuse_before_touching_a_device():
    f1 = np.zeros((8, 10), np.float32)
    f4 = np.zeros((8, 10, 4), np.float32)
    u1 = np.zeros((8, 10), np.uint8)
    u3 = np.zeros((8, 10, 3), np.uint8)
    u4 = np.zeros((8, 10, 4), np.uint8)
    vf1, vf4, vu1, vu3, vu4 = _view(f1, F.alpha_f32), _view(f4, F.rgba_f32), _view(u1, F.alpha_u8), _view(u3, F.rgb_u8), _view(u4, F.rgba_u8)
    r = C.byref
    # blur: null, format, radius 0, radius past half the smaller extent
    assert "null" in _refused("visp_image_blur", None, None, 1)
    assert "format" in _refused("visp_image_blur", None, r(vu1[0]), 1)
    assert "radius" in _refused("visp_image_blur", None, r(vf1[0]), 0)
    assert "radius" in _refused("visp_image_blur", None, r(vf4[0]), 5)  # min(10, 8) / 2 = 4
    # erosion
    assert "null" in _refused("visp_image_erosion", None, None, 1)
    assert "format" in _refused("visp_image_erosion", None, r(vf4[0]), 1)
    assert "radius" in _refused("visp_image_erosion", None, r(vu1[0]), 0)
    # estimator: formats, extent mismatch, radius
    small = _view(np.zeros((8, 9), np.float32), F.alpha_f32)
    assert "null" in _refused("visp_image_estimate_foreground", None, r(vf4[0]), None, 3)
    assert "format" in _refused("visp_image_estimate_foreground", None, r(vu4[0]), r(vf1[0]), 3)
    assert "format" in _refused("visp_image_estimate_foreground", None, r(vf4[0]), r(vu1[0]), 3)
    assert "extents differ" in _refused("visp_image_estimate_foreground", None, r(vf4[0]), r(small[0]), 3)
    assert "radius" in _refused("visp_image_estimate_foreground", None, r(vf4[0]), r(vf1[0]), 30)
    assert "radius" in _refused("visp_image_estimate_foreground", None, r(vf4[0]), r(vf1[0]), 0)
    # composite
    small_u1 = _view(np.zeros((8, 9), np.uint8), F.alpha_u8)
    assert "null" in _refused("visp_image_alpha_composite", None, r(vu4[0]), None, r(vu1[0]))
    assert "format" in _refused("visp_image_alpha_composite", None, r(vu3[0]), r(vu3[0]), r(vu1[0]))
    assert "format" in _refused("visp_image_alpha_composite", None, r(vu4[0]), r(vu1[0]), r(vu1[0]))
    assert "format" in _refused("visp_image_alpha_composite", None, r(vu4[0]), r(vu3[0]), r(vu4[0]))
    assert "extents differ" in _refused("visp_image_alpha_composite", None, r(vu4[0]), r(vu3[0]), r(small_u1[0]))
    # the host-only pair
    assert "null" in _refused("visp_image_set_alpha", r(vu4[0]), None)
    assert "4-channel" in _refused("visp_image_set_alpha", r(vu3[0]), r(vu1[0]))
    assert "alpha_u8" in _refused("visp_image_set_alpha", r(vu4[0]), r(vu4[0]))
    assert "extents differ" in _refused("visp_image_set_alpha", r(vu4[0]), r(small_u1[0]))
    assert "null" in _refused("visp_image_to_mask", None)
    assert "u8" in _refused("visp_image_to_mask", r(vf1[0]))
    # a view whose rows are shorter than its pixels
    bad = L.ImageView(10, 8, 5, F.alpha_f32.value, f1.ctypes.data)
    assert "stride" in _refused("visp_image_blur", None, r(bad), 1)


def test_device_batch_entries_refuse_before_touching_a_device():
    api = L.get_lib()
    p = 0x10000  # never dereferenced: every call below is refused by its argument checks

    def refused(*a):
        assert api.visp_image_estimate_foreground_batch_device(None, *a, None) == 0
        return api.visp_get_last_error().decode()

    assert "null" in refused(None, F.rgb_u8.value, p, 1, 64, 64, 30, p, F.rgba_u8.value)
    assert "null" in refused(p, F.rgb_u8.value, None, 1, 64, 64, 30, p, F.rgba_u8.value)
    assert "format" in refused(p, F.alpha_u8.value, p, 1, 64, 64, 30, p, F.rgba_u8.value)
    assert "format" in refused(p, F.rgb_u8.value, p, 1, 64, 64, 30, p, F.rgb_u8.value)
    assert "radius" in refused(p, F.rgb_u8.value, p, 1, 64, 64, 33, p, F.rgba_u8.value)
    assert "radius" in refused(p, F.rgb_u8.value, p, 1, 64, 60, 0, p, F.rgba_u8.value)
    assert "batch" in refused(p, F.rgb_u8.value, p, 0, 64, 64, 30, p, F.rgba_u8.value)
    assert "32-bit" in refused(p, F.rgb_u8.value, p, 64, 4096, 4096, 30, p, F.rgba_u8.value)
    # the cutout entries need a model first
    assert api.visp_birefnet_cutout_batch_device(None, p, 1, 64, 64, 30, p, None) == 0
    assert "null" in api.visp_get_last_error().decode()
    assert api.visp_birefnet_cutout_batch_host(None, p, 1, 64, 64, 30, p) == 0


def test_launchers_refuse_bad_arguments():
    """null and misaligned pointers, an illegal radius, outputs that overlap inputs, extents past 32-bit indexing: refused with a text, nothing launched."""
    api = L.get_lib()
    a, b, c, d, e = 0x100000, 0x200000, 0x300000, 0x400000, 0x500000  # device addresses that are never used: every call is refused

    def err(ok):
        assert ok == 0
        return api.vx_last_error().decode()

    blur = api.vx_box_blur_f32
    assert "null" in err(blur(None, 8, b, c, 8, 1, 8, 8, 1, 1, None))
    assert "null" in err(blur(a, 8, None, c, 8, 1, 8, 8, 1, 1, None))
    assert "channels" in err(blur(a, 8, b, c, 8, 1, 8, 8, 3, 1, None))
    assert "misaligned" in err(blur(a + 2, 8, b, c, 8, 1, 8, 8, 1, 1, None))
    assert "misaligned" in err(blur(a + 4, 32, b, c, 32, 1, 8, 8, 4, 1, None))  # rgba needs 16 bytes
    assert "misaligned" in err(blur(a, 34, b, c, 32, 1, 8, 8, 4, 1, None))      # a row stride that is no multiple of the pixel
    assert "radius" in err(blur(a, 8, b, c, 8, 1, 8, 8, 1, 0, None))
    assert "radius" in err(blur(a, 8, b, c, 8, 1, 8, 8, 1, 5, None))
    assert "radius" in err(blur(a, 64, b, c, 64, 1, 8, 64, 1, 5, None))          # the smaller extent decides
    assert "overlap" in err(blur(a, 8, b, a + 64, 8, 1, 8, 8, 1, 1, None))
    assert "overlap" in err(blur(a, 8, a, c, 8, 1, 8, 8, 1, 1, None))
    assert "row strides" in err(blur(a, 7, b, c, 8, 1, 8, 8, 1, 1, None))
    assert "positive" in err(blur(a, 8, b, c, 8, 0, 8, 8, 1, 1, None))
    assert "32-bit" in err(blur(a, 65536, b, c, 65536, 8, 65536, 65536, 1, 1, None))
    for erode in (api.vx_erode_f32, api.vx_erode_u8):
        assert "null" in err(erode(None, 8, c, 8, 1, 8, 8, 1, None))
        assert "radius" in err(erode(a, 8, c, 8, 1, 8, 8, 0, None))
        assert "radius" in err(erode(a, 8, c, 8, 1, 8, 8, 65, None))
        assert "overlaps" in err(erode(a, 8, a + 8, 8, 1, 8, 8, 1, None))
        assert "32-bit" in err(erode(a, 65536, c, 65536, 8, 65536, 65536, 1, None))
    assert "misaligned" in err(api.vx_erode_f32(a + 1, 8, c, 8, 1, 8, 8, 1, None))
    stage = api.vx_foreground_stage
    ok_args = dict(img=a, fmt=3, fg=None, bg=None, mask=b, planes=c, out=d, out_fmt=0, bg_out=e, B=1, h=64, w=64, r=30, passes=3)

    def st(**kw):
        v = {**ok_args, **kw}
        return stage(v["img"], v["fmt"], v["fg"], v["bg"], v["mask"], v["planes"], v["out"], v["out_fmt"], v["bg_out"], v["B"], v["h"], v["w"], v["r"], v["passes"], None)

    assert "passes" in err(st(passes=0))
    assert "passes" in err(st(passes=4))
    assert "null" in err(st(img=None))
    assert "null" in err(st(planes=None))
    assert "together" in err(st(fg=a))
    assert "image format" in err(st(fmt=4))
    assert "output format" in err(st(out_fmt=3))
    assert "misaligned" in err(st(mask=b + 2))
    assert "misaligned" in err(st(fmt=5, img=a + 4))
    assert "misaligned" in err(st(planes=c + 4))
    assert "radius" in err(st(r=33))
    assert "radius" in err(st(r=0))
    assert "overlaps" in err(st(out=a))
    assert "overlaps" in err(st(planes=b + 4096))
    assert "overlap" in err(st(bg_out=d))
    assert "32-bit" in err(st(B=64, h=4096, w=4096))
    comp = api.vx_alpha_composite_u8
    assert "null" in err(comp(a, None, 3, c, d, 64, None))
    assert "channels" in err(comp(a, b, 1, c, d, 64, None))
    assert "misaligned" in err(comp(a + 1, b, 3, c, d, 64, None))
    assert "overlaps" in err(comp(a, b, 3, c, b + 16, 64, None))
    assert "pixels" in err(comp(a, b, 3, c, d, 0, None))
    assert "pixels" in err(comp(a, b, 3, c, d, 1 << 30, None))

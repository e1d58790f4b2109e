"""The float64 references of tests/imgops_ref.py, pinned on implementations that are not ours: the image resize and the LayerNorm on torch, the patches on
the CPU oracle's image_to_patches, the strided resize on the reference the existing resize tests use (tests/deform_ref.py), the gate on a loop in plain
numpy. No GPU."""
import numpy as np
import pytest
import torch

import deform_ref
import imgops_ref as R
from oracle import oracle

RESIZE_CASES = [((12, 8), (6, 4)), ((13, 9), (5, 4)), ((1, 1), (3, 2)), ((5, 3), (1, 1)), ((7, 5), (16, 11))]  # (W, H) -> (w, h); the last one upscales


@pytest.mark.parametrize("src,dst", RESIZE_CASES, ids=lambda c: "x".join(map(str, c)))
@pytest.mark.parametrize("C", [3, 4])
def test_image_resize_is_torch_bilinear_align_corners(src, dst, C):
    rng = np.random.default_rng(src[0] * 10 + C)
    x = rng.standard_normal((2, src[1], src[0], C))
    want = torch.nn.functional.interpolate(torch.from_numpy(x).permute(0, 3, 1, 2), size=(dst[1], dst[0]), mode="bilinear", align_corners=True).permute(0, 2, 3, 1).numpy()
    got = R.image_bilinear_ac(x, dst[1], dst[0])
    assert got.shape == want.shape == (2, dst[1], dst[0], C)
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-13)
    # the same formula rounded to f32 at every step: what the kernel's error is measured against (a few f32 ulps of values of order 1)
    f32 = R.image_bilinear_ac(x.astype(np.float32), dst[1], dst[0], np.float32)
    assert f32.dtype == np.float32 and np.abs(f32 - R.image_bilinear_ac(x.astype(np.float32), dst[1], dst[0])).max() < 2e-5


def test_image_resize_edge_rules():
    x = np.arange(2 * 3 * 5 * 3, dtype=np.float64).reshape(2, 3, 5, 3)
    np.testing.assert_array_equal(R.image_bilinear_ac(x, 1, 1), x[:, :1, :1])       # out 1: coordinate 0
    np.testing.assert_array_equal(R.image_bilinear_ac(x, 3, 5), x)                   # the identity
    np.testing.assert_array_equal(R.image_bilinear_ac(x[:, :1, :1], 2, 3), np.broadcast_to(x[:, :1, :1], (2, 2, 3, 3)))  # a 1 x 1 source: both taps clamp
    np.testing.assert_array_equal(R.image_bilinear_ac(x, 2, 2), x[:, ::2, ::4])      # align_corners: the corners map onto the corners


@pytest.mark.parametrize("IW,IH,w,h", [(24, 16, 6, 4), (16, 16, 2, 2), (24, 8, 6, 4), (8, 8, 8, 8)])
@pytest.mark.parametrize("C", [3, 4])
def test_patches_are_the_oracles(IW, IH, w, h, C):
    rng = np.random.default_rng(IW + C)
    x = rng.standard_normal((2, IH, IW, C)).astype(np.float32)
    got = R.image_patches(x, h, w)
    assert got.shape == (2, h, w, (IW // w) * (IH // h) * C)
    for b in range(2):
        np.testing.assert_array_equal(got[b], oracle.image_to_patches(x[b], w, h))
    gw, gh = IW // w, IH // h  # the pattern in words, on single elements
    for gx, gy, c, py, px in ((0, 0, 0, 0, 0), (gw - 1, gh - 1, C - 1, h - 1, w - 1), (gw // 2, 0, 1, h // 2, 0)):
        assert got[1, py, px, gx + gw * (gy + gh * c)] == x[1, gy * h + py, gx * w + px, c]
    with pytest.raises(AssertionError, match="Grid must divide image size"):
        R.image_patches(x, h, w + 1)


@pytest.mark.parametrize("C,Cg", [(8, 8), (64, 16), (72, 16)])
def test_gate_is_p_times_the_rounded_sigmoid(C, Cg):
    rng = np.random.default_rng(C)
    p, a, w, bias = rng.standard_normal((35, C)), rng.standard_normal((35, Cg)), rng.standard_normal(Cg), 0.3
    got = R.pixel_gate(p, a, w, bias)
    for r in (0, 17, 34):
        s = bias
        for k in range(Cg):
            s += a[r, k] * w[k]
        g = float(np.float16(1.0 / (1.0 + np.exp(-s))))
        np.testing.assert_allclose(got[r], p[r] * g, rtol=1e-15)
    assert np.abs(got).max() <= np.abs(p).max()  # a gate in [0, 1]


@pytest.mark.parametrize("src,dst", [((12, 8), (6, 4)), ((3, 2), (6, 4)), ((1, 1), (6, 4)), ((6, 4), (1, 1))])
def test_strided_resize_reference_is_the_resize_tests_reference(src, dst):
    x = np.random.default_rng(src[0]).standard_normal((2, src[1], src[0], 16))
    np.testing.assert_allclose(R.bilinear_ac(x, dst[1], dst[0]), deform_ref.bilinear_ac(x, dst[1], dst[0]), rtol=0, atol=1e-14)


@pytest.mark.parametrize("C", [8, 72, 256, 1024])
def test_layer_norm_is_torchs(C):
    rng = np.random.default_rng(C)
    x, w, b = rng.standard_normal((5, C)) * 3 + 1, rng.standard_normal(C), rng.standard_normal(C)
    want = torch.nn.functional.layer_norm(torch.from_numpy(x), (C,), torch.from_numpy(w), torch.from_numpy(b), 1e-5).numpy()
    np.testing.assert_allclose(R.layer_norm(x, w, b, 1e-5), want, rtol=0, atol=1e-12)


def test_f16_floor():
    want = np.array([1.0, 1.0 + 2.0 ** -12, 0.5])
    assert R.f16_floor(want) == pytest.approx(2.0 ** -12 / (1.0 + 2.0 ** -12))

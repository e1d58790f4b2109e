"""Pins tests/deform_ref.py (the float64 reference the GPU tests of the deformable conv compare against) without a GPU: against the CPU
oracle's vo_deform_conv2d_nhwc (f32; the convention both follow) and against torch's plain convolution in float64."""
import numpy as np
import pytest
import torch

import deform_ref as R
from oracle import oracle


def _rel(got, want):
    return float(np.abs(np.asarray(got, np.float64) - want).max() / np.abs(want).max())


def _operands(k, seed, B=2, h=9, w=11, C=16, Cout=24):
    rng = np.random.default_rng(seed)
    taps = k * k
    x = R.f16(rng.standard_normal((B, h, w, C)))
    wgt = R.f16(rng.standard_normal((Cout, k, k, C)) / np.sqrt(taps * C))
    off = R.f16(rng.standard_normal((B, h, w, 2 * taps)) * 1.2)
    mask = R.f16(2.0 * R.sigmoid(rng.standard_normal((B, h, w, taps))))
    # planted positions (integer + f16 offset: exact in f32): far outside, on an integer, exactly -1 and exactly H (both excluded), H - 1/2
    pad = k // 2
    off[0, 0, 0, 0:2] = [-30, 4]
    off[0, 2, 3, 0:2] = [1, -2]
    off[0, 0, 5, 0] = -1 - (0 - pad)
    off[0, h - 1, 5, 0] = h - (h - 1 - pad)
    off[1, h - 1, 2, 0] = (h - 0.5) - (h - 1 - pad)
    return x, wgt, off, mask


@pytest.mark.parametrize("k", [1, 3, 7])
@pytest.mark.parametrize("masked", [False, True])
def test_reference_matches_the_oracle(k, masked):
    """rel_err < 2e-4 = K 2^-24 at K = 3136, the worst case of the oracle's f32 accumulation; about 1e-6 is expected."""
    x, wgt, off, mask = _operands(k, k)
    want = R.deform_conv2d(x, wgt, off, mask if masked else None, k // 2)
    got = np.stack([oracle.deform_conv2d_nhwc(x[b], wgt, off[b], mask[b] if masked else None, 1, k // 2) for b in range(x.shape[0])])
    err = _rel(got, want)
    print(f"deform_ref vs oracle k={k} masked={masked}: rel_err {err:.3g}")
    assert err < 2e-4, err


@pytest.mark.parametrize("k,pad", [(1, 0), (3, 1), (7, 3), (3, 0)])
def test_zero_offsets_and_a_mask_of_ones_is_a_plain_convolution(k, pad):
    x, wgt, off, mask = _operands(k, 10 + k)
    B, h, w, _ = x.shape
    oh, ow = h + 2 * pad - k + 1, w + 2 * pad - k + 1
    zeros, ones = np.zeros((B, oh, ow, 2 * k * k)), np.ones((B, oh, ow, k * k))
    want = torch.nn.functional.conv2d(torch.from_numpy(x).permute(0, 3, 1, 2), torch.from_numpy(wgt).permute(0, 3, 1, 2), padding=pad).permute(0, 2, 3, 1).numpy()
    assert _rel(R.deform_conv2d(x, wgt, zeros, ones, pad), want) < 1e-12
    assert _rel(R.deform_conv2d(x, wgt, zeros, None, pad), want) < 1e-12
    assert _rel(R.conv2d(x, wgt, None, pad), want) < 1e-12


def test_the_strict_inequality_and_the_half_outside_row():
    """One channel, one tap: samples exactly at -1 and at H give zero, a sample at H - 1/2 gives half of the last row."""
    x = np.arange(1.0, 13.0).reshape(1, 4, 3, 1)
    for py, want in [(-1.0, 0.0), (4.0, 0.0), (3.5, 0.5 * x[0, 3, 1, 0]), (-0.5, 0.5 * x[0, 0, 1, 0]), (2.0, x[0, 2, 1, 0])]:
        got = R.deform_sample(x, np.full((1, 1, 1), py), np.full((1, 1, 1), 1.0))[0, 0, 0, 0]
        assert got == want, (py, got, want)


def test_glue_references_match_the_oracle():
    rng = np.random.default_rng(3)
    x = R.f16(rng.standard_normal((2, 12, 8, 8)))
    # the oracle forms the source coordinate in f32 (two roundings, |coordinate| <= 23: off by up to 2 x 23 x 2^-24 = 2.7e-6 pixels), and neighbouring
    # values differ by up to about twice the largest value: 1e-5 of it
    for oh, ow in [(3, 2), (24, 16), (12, 8)]:
        assert _rel(oracle.interpolate_nhwc(x, (oh, ow), "bilinear", True), R.bilinear_ac(x, oh, ow)) < 1e-5
    one = R.f16(rng.standard_normal((2, 1, 1, 8)))
    np.testing.assert_allclose(R.bilinear_ac(one, 4, 6), np.broadcast_to(one, (2, 4, 6, 8)), rtol=1e-15)  # a (1 - f) + a f
    w = R.f16(rng.standard_normal((5, 3, 3, 8)) * 0.2)
    assert _rel(oracle.conv2d_nhwc(x, w, None, 1, 1), R.conv2d(x, w, None, 1)) < 1e-5
    np.testing.assert_allclose(R.mean_2d(x)[:, 0, 0], x.reshape(2, -1, 8).mean(1), rtol=1e-13)

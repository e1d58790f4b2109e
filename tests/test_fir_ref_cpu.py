"""tests/fir_ref.py, the float64 reference of the MI-GAN graph tests, pinned to the literal node chain in torch (repeat_interleave x2, the mask tile,
conv2d(groups = C, padding = 2), crop) and to tests/migan_ref.py::upsample, to 1e-6, on the symmetric filter of the trained file and on an asymmetric one
(asymmetric_fir: flipped or transposed taps show); clamp and lrelu_agc to torch."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import fir_ref as R
import migan_ref

CASES = [(2, 1, 1, 8), (1, 2, 3, 24), (1, 5, 9, 16), (2, 4, 4, 8), (1, 3, 4, 8)]  # (B, h, w, C): the cases of tests/test_gpu_graph_migan.py


@pytest.mark.parametrize("case", CASES)
def test_upfirdn2x_equals_the_literal_chain(case):
    B, h, w, C = case
    rng = np.random.default_rng(sum(case))
    x = R.f16(rng.standard_normal(case))
    fir = R.f16(R.perturbed_fir(rng, C))
    t = torch.from_numpy(x).permute(0, 3, 1, 2)
    up = t.repeat_interleave(2, 2).repeat_interleave(2, 3)
    tile = torch.tensor([[1.0, 0.0], [0.0, 0.0]], dtype=torch.float64).repeat(h, w)
    k = torch.from_numpy(fir).permute(2, 0, 1)[:, None]  # [C, 1, 4, 4]
    want = F.conv2d(up * tile, k, padding=2, groups=C)[:, :, :2 * h, :2 * w].permute(0, 2, 3, 1).numpy()
    got = R.upfirdn2x(x, fir)
    assert got.shape == (B, 2 * h, 2 * w, C)
    np.testing.assert_allclose(got, want, rtol=1e-6, atol=1e-6)
    ref = migan_ref.upsample(x.astype(np.float32), np.ascontiguousarray(fir.transpose(2, 0, 1)[:, None]).astype(np.float32))
    np.testing.assert_allclose(got, ref, rtol=1e-6, atol=1e-6)  # (migan_ref computes in f32)


@pytest.mark.parametrize("case", CASES)
def test_upfirdn2x_equals_migan_ref_on_an_asymmetric_filter(case):
    """the symmetric filter above satisfies f[ky][kx] == f[kx][ky] == f[3 - ky][3 - kx]: a reference that flipped or transposed its taps would pass there"""
    B, h, w, C = case
    rng = np.random.default_rng(100 + sum(case))
    x = R.f16(rng.standard_normal(case))
    sym, fir = R.f16(R.perturbed_fir(rng, C)), R.f16(R.asymmetric_fir(rng, C))
    flipped, transposed = fir[::-1, ::-1], fir.transpose(1, 0, 2)
    assert np.array_equal(sym, sym[::-1, ::-1]) and np.array_equal(sym, sym.transpose(1, 0, 2))
    # every channel tells its taps apart: a flip or a transpose moves a tap by more than a tenth of the largest one
    assert (np.abs(fir - flipped).max((0, 1)) > 0.1 * fir.max((0, 1))).all() and (np.abs(fir - transposed).max((0, 1)) > 0.1 * fir.max((0, 1))).all()
    got = R.upfirdn2x(x, fir)
    ref = migan_ref.upsample(x.astype(np.float32), np.ascontiguousarray(fir.transpose(2, 0, 1)[:, None]).astype(np.float32))
    np.testing.assert_allclose(got, ref, rtol=1e-6, atol=1e-6)
    t = torch.from_numpy(x).permute(0, 3, 1, 2)
    tile = torch.tensor([[1.0, 0.0], [0.0, 0.0]], dtype=torch.float64).repeat(h, w)
    k = torch.from_numpy(fir.copy()).permute(2, 0, 1)[:, None]
    want = F.conv2d(t.repeat_interleave(2, 2).repeat_interleave(2, 3) * tile, k, padding=2, groups=C)[:, :, :2 * h, :2 * w].permute(0, 2, 3, 1).numpy()
    np.testing.assert_allclose(got, want, rtol=1e-6, atol=1e-6)
    assert R.rel_err(R.upfirdn2x(x, flipped), got) > 0.02 and R.rel_err(R.upfirdn2x(x, transposed), got) > 0.02


def test_upfirdn2x_epilogue_order():
    rng = np.random.default_rng(3)
    x, fir = R.f16(rng.standard_normal((1, 2, 2, 8)) * 200), R.f16(R.perturbed_fir(rng, 8))
    plane, res = rng.standard_normal((4, 4)), R.f16(rng.standard_normal((1, 4, 4, 8)))
    raw = R.upfirdn2x(x, fir)
    want = np.clip(F.leaky_relu(torch.from_numpy(raw + plane[None, :, :, None]), 0.2).numpy() * np.sqrt(2.0), -256, 256) + res
    np.testing.assert_allclose(R.upfirdn2x(x, fir, plane, res, (np.sqrt(2.0), 256.0)), want, rtol=1e-12)
    assert 0.0 < R.clamped_fraction(x, fir, plane, (np.sqrt(2.0), 256.0)) < 1.0


def test_clamp_lrelu_agc_plane_and_depthwise_equal_torch():
    v = np.concatenate([R.f16(np.random.default_rng(0).standard_normal(1000) * 300), [60000.0, -60000.0, 256.0, -256.0, 255.9, -255.9, 0.0, -0.0, np.inf, -np.inf]])
    np.testing.assert_array_equal(R.clamp(v, -256.0, 256.0), torch.clamp(torch.from_numpy(v), -256.0, 256.0).numpy())
    assert np.signbit(R.clamp(np.array([-0.0]), -1.0, 1.0))[0]
    f = v[np.isfinite(v)]
    want = torch.clamp(F.leaky_relu(torch.from_numpy(f), 0.2) * np.sqrt(2.0), -256.0, 256.0).numpy()
    np.testing.assert_allclose(R.lrelu_agc(f), want, rtol=1e-12)
    np.testing.assert_allclose(migan_ref.lrelu_agc(f.astype(np.float32)), want, rtol=1e-6)
    rng = np.random.default_rng(1)
    a, b = rng.standard_normal((2, 3, 5, 8)), rng.standard_normal((3, 5))
    for op, fn in ((R.ADD, np.add), (R.MUL, np.multiply), (R.SUB, np.subtract)):
        np.testing.assert_array_equal(R.plane_binary(op, a, b), fn(a, b[None, :, :, None]))
    x, w, bias = rng.standard_normal((2, 5, 7, 8)), rng.standard_normal((3, 3, 8)), rng.standard_normal(8)
    for stride, pad, k in ((1, 1, 3), (2, 1, 4), (1, 2, 4)):
        wk = rng.standard_normal((k, k, 8)) if k != 3 else w
        want = F.conv2d(torch.from_numpy(x).permute(0, 3, 1, 2), torch.from_numpy(wk).permute(2, 0, 1)[:, None], torch.from_numpy(bias), stride, pad, groups=8)
        np.testing.assert_allclose(R.depthwise(x, wk, bias, stride, pad), want.permute(0, 2, 3, 1).numpy(), rtol=1e-9, atol=1e-9)

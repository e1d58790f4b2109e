"""tests/pool_ref.py, the float64 reference of the pooling / SiLU / softmax tests, pinned to torch: max_pool2d (padding never wins), avg_pool2d at pad 0,
silu and softmax, at every case the GPU tests use, to 1e-6."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import pool_ref as R


def _case_input(i):
    kind, k, s, pad, C, H, W, B = R.POOL_CASES[i]
    return R.f16(np.random.default_rng(300 + i).standard_normal((B, H, W, C)))


@pytest.mark.parametrize("i", range(len(R.POOL_CASES)))
def test_pool2d_equals_torch(i):
    kind, k, s, pad, C, H, W, B = R.POOL_CASES[i]
    x = _case_input(i)
    t = torch.from_numpy(x).permute(0, 3, 1, 2)
    want = F.max_pool2d(t, k, s, pad) if kind == R.MAX else F.avg_pool2d(t, k, s, 0)
    got = R.pool2d(x, kind, k, s, pad)
    assert got.shape == (B, R.out_extent(H, k, s, pad), R.out_extent(W, k, s, pad), C)
    np.testing.assert_allclose(got, want.permute(0, 2, 3, 1).numpy(), rtol=1e-6, atol=1e-6)
    if kind == R.MAX:  # the maximum of f16 values is one of them
        np.testing.assert_array_equal(got, R.f16(got))


def test_pool2d_refuses_what_the_graph_refuses():
    with pytest.raises(ValueError, match="does not fit"):
        R.pool2d(np.zeros((3, 2, 19, 40)), R.AVG, 3, 1, 0)
    with pytest.raises(ValueError, match="padding"):
        R.pool2d(np.zeros((1, 4, 4, 8)), R.AVG, 3, 1, 1)


def test_silu_and_softmax_equal_torch():
    rng = np.random.default_rng(1)
    x = np.concatenate([R.f16(rng.standard_normal(500) * 4), [-20.0, -0.0, 11.0, 60000.0]])
    np.testing.assert_allclose(R.silu(x), F.silu(torch.from_numpy(x)).numpy(), rtol=1e-6, atol=1e-6)
    assert np.isfinite(R.silu(x)).all()
    rows = R.f16(rng.standard_normal((7, 80)) * 3)
    rows[0] = R.f16(np.linspace(-60000, 60000, 80))
    rows[1] = 3.5
    np.testing.assert_allclose(R.softmax(rows), torch.softmax(torch.from_numpy(rows), -1).numpy(), rtol=1e-6, atol=1e-6)
    proj = np.arange(80.0)
    np.testing.assert_allclose(R.softmax_expect(rows, proj), (torch.softmax(torch.from_numpy(rows), -1) * torch.from_numpy(proj)).sum(-1).numpy(), rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(R.sum_rows(rows)[:, 0], torch.from_numpy(rows).sum(-1).numpy(), rtol=1e-6, atol=1e-6)
    assert abs(R.softmax_expect(rows[1], proj) - 39.5) < 1e-9 and R.f16_floor(np.array([1.0, 1.0 + 2.0 ** -12])) > 0

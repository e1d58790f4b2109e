"""tests/sam_prompts_ref.py pinned without a device: the mask post-processing against the oracle's sam_process_mask, the iou head against torch
linears in float64, the choice rule on ties, and the point grid / prompt packing of the Python face."""
import numpy as np
import pytest
import torch

from oracle import oracle as O
from tests import sam_prompts_ref as R


def _h(a):
    return a.astype(np.float16).astype(np.float32)


@pytest.mark.parametrize("tw,th", [(1024, 1024), (640, 480), (333, 517)])
def test_process_mask_is_the_oracles(tw, th):
    rng = np.random.default_rng(tw)
    yy, xx = np.meshgrid(np.linspace(-3, 3, 256), np.linspace(-3, 3, 256), indexing="ij")
    mask = _h(np.sin(2 * xx) * np.cos(3 * yy) + 0.3 * rng.standard_normal((256, 256)))
    got, want = R.process_mask(mask, tw, th), O.sam_process_mask(mask, tw, th)
    assert got.shape == want.shape == (th, tw) and got.dtype == np.uint8
    assert (got != want).mean() < 1e-5, (got != want).mean()  # the bound tests/test_gpu_tinyvit.py holds the single-prompt kernel to


def test_process_masks_reads_the_chosen_plane_of_each_prompt():
    rng = np.random.default_rng(5)
    planes = _h(rng.standard_normal((3, 4, 32, 32)))
    chosen = np.array([2, 0, 3])
    got = R.process_masks(planes, chosen, 40, 24, image_size=64)
    assert got.shape == (3, 24, 40)
    for p in range(3):
        np.testing.assert_array_equal(got[p], R.process_mask(planes[p, chosen[p]], 40, 24, image_size=64))
    assert not np.array_equal(got[0], R.process_mask(planes[0, 0], 40, 24, image_size=64))  # a seeded defect: plane 0 for everyone
    np.testing.assert_array_equal(R.process_masks(planes, [7, -1, 3], 40, 24, 64), R.process_masks(planes, [3, 0, 3], 40, 24, 64))


def test_interpolate_identity_and_constant():
    rng = np.random.default_rng(6)
    a = rng.standard_normal((9, 13)).astype(np.float32)
    np.testing.assert_array_equal(R.interpolate(a, 13, 9, 13, 9), a)
    np.testing.assert_array_equal(R.interpolate(np.full((5, 5), 2.5, np.float32), 5, 5, 17, 11), np.full((11, 17), 2.5, np.float32))


@pytest.mark.parametrize("case", R.iou_head_cases(), ids=lambda c: c[0])
def test_iou_head_against_torch_linears(case):
    _, tokens, ws, bs = case
    x = torch.from_numpy(tokens.astype(np.float64))
    for l in range(3):
        x = torch.nn.functional.linear(x, torch.from_numpy(ws[l].astype(np.float64)), torch.from_numpy(bs[l].astype(np.float64)))
        if l < 2:
            x = torch.relu(x)
    want = x.numpy()
    got = R.iou_head(tokens, ws, bs)
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-12)
    f32 = R.iou_head_f32_ascending(tokens, ws, bs)
    assert f32.dtype == np.float32
    err = np.abs(f32 - want).max()
    assert 0 < err < 1e-4, err  # float32 sums of 256 terms of order 1: a few 1e-6; exactly 0 would mean the float32 path ran in float64


def test_cases_hold_the_tie_and_the_near_tie():
    cases = {c[0]: c for c in R.iou_head_cases()}
    _, tokens, ws, bs = cases["tie"]
    want = R.iou_head(tokens, ws, bs)
    assert np.array_equal(want[:, 0], want[:, 1]) and (want[:, 0] > want[:, 2]).all()
    assert (R.choose(want) == 0).all()
    _, tokens, ws, bs = cases["close"]
    want = R.iou_head(tokens, ws, bs)
    np.testing.assert_allclose(want[:, 1] - want[:, 0], 1e-4, rtol=0, atol=1e-8)
    assert (R.choose(want) == 1).all()


def test_choose_takes_the_first_of_equal_maxima_and_ignores_the_fourth():
    iou = np.array([[0.5, 0.5, 0.1, 9.0], [0.1, 0.7, 0.7, 9.0], [0.3, 0.3, 0.3, 0.0], [0.1, 0.2, 0.3, 0.0], [-1.0, -2.0, -1.0, 5.0]], np.float32)
    np.testing.assert_array_equal(R.choose(iou), [0, 1, 0, 2, 0])
    assert R.choose(iou).dtype == np.int32


def test_point_grid_and_prompt_packing():
    from visioncpp_amd import vision
    g = vision.sam_point_grid(32, 1024, 1024)
    assert g.shape == (1024, 2) and g.dtype == np.int32
    np.testing.assert_array_equal(g[0], [16, 16])
    np.testing.assert_array_equal(g[1], [48, 16])     # x runs first
    np.testing.assert_array_equal(g[-1], [1008, 1008])
    g = vision.sam_point_grid(3, 640, 480)
    np.testing.assert_array_equal(g[:, 0].reshape(3, 3)[0], [106, 320, 533])
    np.testing.assert_array_equal(g[:, 1].reshape(3, 3)[:, 0], [80, 240, 400])
    p, k = vision.Model._sam_prompt_arrays([[1, 2], [3, 4, 5, 6], [7, 8, 9]])
    np.testing.assert_array_equal(k, [2, 4, 3])
    np.testing.assert_array_equal(p, [[1, 2, 0, 0], [3, 4, 5, 6], [7, 8, 9, 0]])


@pytest.mark.parametrize("B,n,Tk", [(1, 96, 7), (2, 40, 8), (2, 33, 3)])
def test_i2t_against_torch(B, n, Tk):
    """the i2t step against torch's scaled_dot_product_attention, linear and layer_norm in float64"""
    F = torch.nn.functional
    c = R.i2t_case(B, n, Tk, seed=n + Tk)
    tt = {k: torch.from_numpy(np.asarray(v).astype(np.float64)) for k, v in c.items()}
    heads = lambda a: a.reshape(B, -1, 8, 16).transpose(1, 2)
    ao = F.scaled_dot_product_attention(heads(tt["q"]), heads(tt["k_tok"]), heads(tt["v_tok"])).transpose(1, 2).reshape(B, n, 128)
    x = tt["K"] + F.linear(ao, tt["wo"], tt["bo"])
    want = F.layer_norm(x, (256,), tt["ln_w"], tt["ln_b"], eps=1e-5)
    got, got1 = R.i2t(**c)
    np.testing.assert_allclose(got, want.numpy(), rtol=0, atol=1e-11)
    np.testing.assert_allclose(got1, (want + tt["pe"]).numpy(), rtol=0, atol=1e-11)
    assert R.i2t(**{**c, "pe": None})[1] is None
    # seeded defects: the prompt's own tokens matter, and so does the head split
    other = dict(c, k_tok=c["k_tok"][::-1].copy()) if B > 1 else dict(c, k_tok=c["k_tok"][:, ::-1].copy())
    assert np.abs(R.i2t(**other)[0] - got).max() > 1e-3
    assert np.abs(R.i2t(**c, heads=4)[0] - got).max() > 1e-3

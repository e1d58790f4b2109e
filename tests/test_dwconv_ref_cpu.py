"""Pins tests/dwconv_ref.py (the float64 references the GPU tests of the depthwise conv and of the TinyViT block compare against) without a GPU:
against the CPU oracle's vo_conv2d_depthwise_nhwc and vo_tinyvit_block (f32), and against torch's grouped convolution in float64.

Measured agreement (largest error over largest value): depthwise_conv2d against the oracle 7.4e-8 .. 2.3e-7 over the six (k, stride, pad) below with
k > 1 and 8.5e-10 at k = 1 (f32 roundings of a sum of at most 49 products); against torch float64 below 1e-14; tinyvit_block against the oracle's f32
block 1.5e-7 (T = 49, map padded 32 -> 35) and 1.9e-7 (T = 196, 16 -> 28)."""
import numpy as np
import pytest
import torch

import dwconv_ref as R
from oracle import oracle
from visioncpp_amd import synth

KSP = [(3, 1, 1), (3, 2, 1), (4, 1, 2), (4, 2, 1), (5, 1, 2), (7, 1, 3), (1, 1, 0)]


def _operands(k, seed, B=2, H=7, W=10, C=16):
    rng = np.random.default_rng(seed)
    return R.f16(rng.standard_normal((B, H, W, C))), R.f16(rng.standard_normal((k, k, C)) / k), R.f16(rng.standard_normal(C) * 0.1)


@pytest.mark.parametrize("k,stride,pad", KSP)
def test_depthwise_reference_matches_the_oracle_and_torch(k, stride, pad):
    """Bound 49 x 2^-24 = 3e-6: the oracle adds at most 49 products in f32."""
    x, w, b = _operands(k, 10 * k + stride)
    want = R.depthwise_conv2d(x, w, b, stride, pad)
    assert want.shape[1:3] == (R.out_extent(7, k, stride, pad), R.out_extent(10, k, stride, pad))
    got = np.stack([oracle.conv2d_depthwise_nhwc(x[i], w, b, stride, pad) for i in range(x.shape[0])])
    err = R.rel_err(got, want)
    print(f"dwconv_ref vs oracle k={k} s={stride} p={pad}: rel_err {err:.3g}")
    assert got.shape == want.shape and err < 3e-6, err
    t = torch.nn.functional.conv2d(torch.from_numpy(x).permute(0, 3, 1, 2), torch.from_numpy(w).permute(2, 0, 1)[:, None], torch.from_numpy(b), stride=stride, padding=pad,
                                   groups=x.shape[3]).permute(0, 2, 3, 1).numpy()
    assert R.rel_err(want, t) < 1e-14
    assert R.rel_err(R.depthwise_conv2d(x, w, None, stride, pad), t - b) < 1e-14


def test_even_kernel_at_pad_2_gives_one_more_column():
    x, w, _ = _operands(4, 1)
    assert R.depthwise_conv2d(x, w, None, 1, 2).shape == (2, 8, 11, 16)  # W + 1, H + 1 (migan.cpp:41-45 slices them off)


def test_the_two_stored_forms_hold_the_same_kernel():
    w = np.arange(3 * 3 * 8, dtype=np.float64).reshape(3, 3, 8)
    a, b = R.kernel_forms(w)
    assert a.shape == (3, 3, 1, 8) and b.shape == (8, 3, 3, 1)
    for ky in range(3):
        for kx in range(3):
            np.testing.assert_array_equal(a[ky, kx, 0], w[ky, kx])
            np.testing.assert_array_equal(b[:, ky, kx, 0], w[ky, kx])


def test_gelu_tanh_matches_the_oracle_form():
    x = np.linspace(-6, 6, 241)
    assert np.abs(oracle.gelu(x.astype(np.float32), oracle.GELU_TANH_F32) - R.gelu_tanh(x)).max() < 1e-6


@pytest.mark.parametrize("layer,res", [(1, 32), (2, 16)])  # T = 49 on a map padded 32 -> 35, T = 196 on 16 -> 28
def test_tinyvit_block_reference_matches_the_oracle(layer, res):
    """Bound 1e-5: a few hundred f32 roundings along the block's chain of products; the measured agreement is in the module docstring."""
    cfg = synth.TINYVIT_MINI
    tensors, conv2d = synth.tinyvit_gguf_tensors(synth.tinyvit_state_dict(cfg, 4))
    om = oracle.Model(tensors, conv2d, "whcn")
    _, dim, _, heads, ws, _ = cfg.layers()[layer]
    prefix = f"enc.layers.{layer}.blocks.0"
    p = {k[len(prefix) + 1:].replace(".c.", "."): np.asarray(v, np.float64) for k, v in tensors.items() if k.startswith(prefix + ".")}
    p["local_conv.weight"] = p["local_conv.weight"][:, :, 0, :]
    rng = np.random.default_rng(layer)
    x = R.f16(rng.standard_normal((2, res * res, dim)))
    want = R.tinyvit_block(p, x, res, heads, ws)
    oracle.tinyvit_set_gelu_modes(oracle.GELU_TANH_F32, oracle.GELU_TANH_F32)
    try:
        got = np.stack([oracle.tinyvit_block(om, prefix, x[i], res, heads, ws) for i in range(2)])
    finally:
        oracle.tinyvit_set_gelu_modes()
    err = R.rel_err(got, want)
    print(f"tinyvit_block ref vs oracle layer {layer}: rel_err {err:.3g}")
    assert err < 1e-5, err

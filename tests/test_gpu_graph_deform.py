"""-m gpu: the deformable conv (csrc/kernels_deform.hip, vx_deform_conv_f16), sigmoid and mean_2d (kernels_graph.hip) and their lowering
against float64 numpy on f16-rounded operands (tests/deform_ref.py); bilinear | align_corners from a 1 x 1 source and to a smaller target;
then one basic_decoder_block (birefnet.cpp:139-145) built through vision.cpp_amd/graph.py against the CPU oracle's squeeze block.

Measured on MI355X (every test prints its figures; DESIGN.md section 15 carries them):
  deformable conv, rel_err against float64 (bound 6e-3, the composed form's: tests/test_gpu_birefnet.py:96): 2.7e-4 .. 4.7e-4 for the op in its three
  mask modes, 3.0e-4 .. 3.9e-4 for aspp_module_deformable as two launches, 5.5e-4 .. 8.5e-4 node by node
  sigmoid 2.4e-4 (2e-3); mean_2d 1.1e-4 / 7.6e-6 at 35 / 5000 pixels (2e-3); bilinear | align_corners 1x1 -> 6x4 exact, 12x8 -> 3x2 1.8e-4 (4e-3)
  decoder block against the oracle: rel_err 4.9e-4, mean 8.6e-5 of the largest value with fused models, 6.6e-4 / 1.1e-4 without (2e-2 / 4e-3);
  against float64 4.5e-4 / 5.9e-4"""
import ctypes as C
import dataclasses
import functools

import numpy as np
import pytest

import deform_ref as R
from oracle import oracle
from visioncpp_amd import _lib as L
from visioncpp_amd import graph as G
from visioncpp_amd import synth, vision

pytestmark = pytest.mark.gpu

from gpu_util import api, dev, empty, rel_err, release, sync  # noqa: E402

DEFORM_BOUND = 6e-3   # the composed form's bound (tests/test_gpu_birefnet.py:96): the same rounding points
SIGMOID_BOUND = 2e-3  # test_mean_broadcast_mul_sigmoid
MEAN_BOUND = 2e-3     # test_mean_broadcast_mul_sigmoid, max abs error on N(0, 1) data
INTERPOLATE_BOUND = 4e-3  # tests/test_gpu_graph.py: the bound of the chain that holds bilinear | align_corners


@pytest.fixture(scope="module")
def device():
    assert api().vx_device_count() > 0, "no HIP device visible: the product path has no CPU fallback"
    return vision.Device.init(vision.Backend.gpu)


@pytest.fixture(autouse=True)
def _release_buffers():
    yield
    release()


# ---- the op ------------------------------------------------------------------------------------------------------------------------------

CASES = [(16, 32, 1, 5, 7, 2),     # a map smaller than a pixel tile, odd extent
         (64, 256, 3, 9, 13, 2),   # 117 pixels per image: no multiple of any tile, full Cout
         (64, 256, 7, 4, 6, 1),    # the kernel is larger than the map: most taps land outside
         (32, 48, 3, 16, 16, 3)]   # Cout no multiple of 32


@functools.lru_cache(maxsize=None)
def _operands(case):
    """x, kernel [Cout, k, k, Cin], offsets [B, h, w, 2 taps], mask, logits, bn scale / bias: the f16 values as float64. Offsets are N(0, 1.2)
    rounded to f16 (tests/test_gpu_birefnet.py:83) with planted values; every position is a small integer plus an f16 value, exact in f32."""
    cin, cout, k, h, w, B = case
    taps, pad = k * k, k // 2
    rng = np.random.default_rng(cin + cout + k)
    x = R.f16(rng.standard_normal((B, h, w, cin)))
    wgt = R.f16(rng.standard_normal((cout, k, k, cin)) / np.sqrt(taps * cin))
    off = R.f16(rng.standard_normal((B, h, w, 2 * taps)) * 1.2)
    last = taps - 1  # tap (k - 1, k - 1)
    off[0, 0, 0, 0:2] = [-30, 4]                          # far outside
    off[0, 2, 3, 0:2] = [1, -2]                           # exactly on an integer coordinate
    off[0, 0, 1, 0] = -1 - (0 - pad)                      # py = -1: excluded by the strict inequality
    off[0, h - 1, 2, 2 * last] = h - (h - 1 - pad + k - 1)        # py = H: excluded
    off[B - 1, h - 1, 3, 2 * last] = (h - 0.5) - (h - 1 - pad + k - 1)  # py = H - 1 + 0.5: one row of corners outside
    off[B - 1, 1, w - 1, 2 * last + 1] = (w - 0.5) - (w - 1 - pad + k - 1)  # px = W - 1 + 0.5
    off[B - 1, 1, 0, 1] = -0.5 - (0 - pad)                # px = -0.5
    logits = R.f16(rng.standard_normal((B, h, w, taps)))
    mask = R.f16(2.0 * R.sigmoid(logits))
    scale = (1 + 0.1 * rng.standard_normal(cout)).astype(np.float32)
    bias = (0.1 * rng.standard_normal(cout)).astype(np.float32)
    for a in (x, wgt, off, logits, mask):
        a.setflags(write=False)
    return x, wgt, off, mask, logits, scale, bias


@pytest.mark.parametrize("mode", ["none", "mask"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c)))
def test_op_through_the_graph(device, case, mode):
    cin, cout, k, h, w, B = case
    x, wgt, off, mask, *_ = _operands(case)
    g = G.Graph(device)
    m = G.ModelRef(g)
    xi, oi = g.input((cin, w, h, B), G.F16, "x"), g.input((2 * k * k, w, h, B), G.F16, "offset")
    mi = g.input((k * k, w, h, B), G.F16, "mask") if mode == "mask" else None
    y = g.output(G.conv_2d_deform(m, xi, g.add_weight("w", wgt), oi, mi, 1, k // 2), "y")
    g.allocate()
    assert g.describe().startswith("deform_conv[mask] " if mi is not None else "deform_conv M=")
    g.set(xi, x); g.set(oi, off)
    if mi is not None:
        g.set(mi, mask)
    g.compute()
    want = R.deform_conv2d(x, wgt, off, mask if mi is not None else None, k // 2)
    err = rel_err(g.get(y), want)
    print(f"conv_2d_deform {case} {mode}: rel_err {err:.3g}")
    assert err < DEFORM_BOUND, err


def _module(g, case, fused):
    """aspp_module_deformable with random offset / modulator kernels; returns (input, output, reference of the whole module). The reference rounds the
    offsets and logits to f16 where the device stores them; where the device's f32 sum rounds to the neighbouring f16 value the sample moves by
    one f16 step of the offset -- the bilinear sample is continuous in it, so no element is left out."""
    cin, cout, k, h, w, B = case
    x, wgt, _, _, _, scale, bias = _operands(case)
    taps, pad = k * k, k // 2
    rng = np.random.default_rng(7 * k + cin)
    w_off = R.f16(rng.standard_normal((2 * taps, k, k, cin)) * 0.6 / np.sqrt(taps * cin))
    b_off = R.f16(rng.standard_normal(2 * taps) * 0.6)
    w_mod = R.f16(rng.standard_normal((taps, k, k, cin)) / np.sqrt(taps * cin))
    b_mod = R.f16(rng.standard_normal(taps) * 0.3)
    for name, a, dt in (("a.conv.offset.weight", w_off, G.F16), ("a.conv.offset.bias", b_off, G.F32), ("a.conv.modulator.weight", w_mod, G.F16),
                        ("a.conv.modulator.bias", b_mod, G.F32), ("a.conv.conv.weight", wgt, G.F16), ("a.bn.weight", scale, G.F32), ("a.bn.bias", bias, G.F32)):
        g.add_weight(name, a, dt)
    xi = g.input((cin, w, h, B), G.F16, "x")
    y = g.output(G.birefnet_aspp_module_deformable(G.ModelRef(g, "a"), xi, pad), "y")
    g.set_fused_models(fused)
    offs = R.f16(R.conv2d(x, w_off, b_off, pad))
    logit = R.f16(R.conv2d(x, w_mod, b_mod, pad))
    want = np.maximum(R.deform_conv2d(x, wgt, offs, 2.0 * R.sigmoid(logit), pad) * scale.astype(np.float64) + bias.astype(np.float64), 0.0)
    return xi, y, x, want


@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c)))
def test_fused_logits_form_through_the_graph(device, case):
    """conv_2d(offset), scale(sigmoid(conv_2d(modulator)), 2), conv_2d_deform, mul, add, relu as two launches; and node by node, as a check of both."""
    got = {}
    for fused in (True, False):
        g = G.Graph(device)
        xi, y, x, want = _module(g, case, fused)
        g.allocate()
        lines = g.describe().splitlines()
        assert (len(lines) - 1 == 2 and lines[0].startswith("deform_offsets") and lines[1].startswith("deform_conv[logits x2][*scale][+bias][relu]")) == fused, lines
        g.set(xi, x)
        g.compute()
        got[fused] = g.get(y)
        err = rel_err(got[fused], want)
        print(f"aspp_module_deformable {case} fused={fused}: rel_err {err:.3g}")
        assert err < DEFORM_BOUND, (fused, err)


@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c)))
def test_launcher_directly(case):
    """vx_deform_conv_f16 in logits mode: offsets and logits side by side in one buffer (leading dimension 3 taps padded to 8), scale, bias and ReLU
    in the epilogue, output rows with a leading dimension; then the plain modes, and the launcher's own refusals."""
    cin, cout, k, h, w, B = case
    x, wgt, off, mask, logits, scale, bias = _operands(case)
    taps, M = k * k, B * h * w
    ldom, ldo = -(-3 * taps // 8) * 8, cout + 8
    om = np.zeros((M, ldom), np.float16)
    om[:, :2 * taps] = off.reshape(M, -1)
    om[:, 2 * taps:3 * taps] = logits.reshape(M, -1)
    wp = np.zeros((-(-cout // 32) * 32, taps * cin), np.float16)
    wp[:cout] = wgt.reshape(cout, -1)
    a = L.DeformConvArgs()
    xd, wd, omd, sd, bd = dev(x.astype(np.float16)), dev(wp), dev(om), dev(scale), dev(bias)
    out = empty(M * ldo * 2)
    a.x, a.B, a.H, a.W, a.Cin = xd.ptr, B, h, w, cin
    a.w, a.Cout, a.k, a.pad = wd.ptr, cout, k, k // 2
    a.offset, a.ld_offset, a.mask, a.ld_mask, a.mask_mode, a.mask_scale = omd.ptr, ldom, omd.ptr + 2 * taps * 2, ldom, 2, 2.0
    a.scale, a.bias, a.relu, a.out, a.ldo = sd.ptr, bd.ptr, 1, out.ptr, ldo
    L.vx_check(api().vx_deform_conv_f16(C.byref(a), None))
    sync()
    got = out.to_numpy(np.float16, (M, ldo)).astype(np.float64)
    assert np.all(got[:, cout:] == 0), "only the first Cout columns of a row are written"
    plain = R.deform_conv2d(x, wgt, off, 2.0 * R.sigmoid(logits), k // 2)
    err = rel_err(got[:, :cout].reshape(B, h, w, cout), np.maximum(plain * scale.astype(np.float64) + bias.astype(np.float64), 0.0))
    print(f"vx_deform_conv_f16 {case} logits + epilogue: rel_err {err:.3g}")
    assert err < DEFORM_BOUND, err
    # no epilogue, the mask as it is (a buffer of its own), then no mask
    md = dev(mask.astype(np.float16))
    a.scale, a.bias, a.relu, a.mask, a.ld_mask, a.mask_mode = None, None, 0, md.ptr, taps, 1
    for mode, want in ((1, R.deform_conv2d(x, wgt, off, mask, k // 2)), (0, R.deform_conv2d(x, wgt, off, None, k // 2))):
        a.mask_mode = mode
        L.vx_check(api().vx_deform_conv_f16(C.byref(a), None))
        sync()
        err = rel_err(out.to_numpy(np.float16, (M, ldo))[:, :cout].astype(np.float64).reshape(B, h, w, cout), want)
        print(f"vx_deform_conv_f16 {case} mask_mode {mode}: rel_err {err:.3g}")
        assert err < DEFORM_BOUND, (mode, err)
    a.ld_offset = 2 * taps - 1
    assert api().vx_deform_conv_f16(C.byref(a), None) == 0 and b"offset rows" in api().vx_last_error()
    a.ld_offset, a.Cin = ldom, cin + 8
    assert api().vx_deform_conv_f16(C.byref(a), None) == 0 and b"multiple of 16" in api().vx_last_error()


# ---- sigmoid, mean_2d, interpolate -------------------------------------------------------------------------------------------------------

def test_sigmoid_on_activations(device):
    rng = np.random.default_rng(2)
    x = R.f16(np.concatenate([rng.standard_normal(2 * 5 * 7 * 24 - 4) * 3, [-20, 20, 0, -0.0]]).reshape(2, 5, 7, 24))
    g = G.Graph(device)
    xi = g.input((24, 7, 5, 2), G.F16, "x")
    odd = g.input((3, 5, 1, 1), G.F16, "odd")  # 15 elements: the scalar tail
    y, yo = g.output(G.sigmoid(G.ModelRef(g), xi), "y"), g.output(G.sigmoid(G.ModelRef(g), odd), "yo")
    g.allocate()
    g.set(xi, x); g.set(odd, x.reshape(-1)[:15])
    g.compute()
    err = max(rel_err(g.get(y), R.sigmoid(x)), rel_err(g.get(yo).reshape(-1), R.sigmoid(x.reshape(-1)[:15])))
    print(f"sigmoid: rel_err {err:.3g}")
    assert err < SIGMOID_BOUND
    f32 = (rng.standard_normal(1000) * 3).astype(np.float32)  # the f32 map a 1x1 conv to one channel leaves
    out = empty(1000 * 2)
    L.vx_check(api().vx_sigmoid_f16(dev(f32).ptr, 1, out.ptr, 1000, None))
    sync()
    assert rel_err(out.to_numpy(np.float16, (1000,)), R.sigmoid(f32)) < SIGMOID_BOUND


@pytest.mark.parametrize("W,H", [(35, 1), (100, 50)])  # n = 35 and 5000 pixels, C = 72: test_mean_broadcast_mul_sigmoid's shapes
def test_mean_2d_is_accurate_and_deterministic(device, W, H):
    rng = np.random.default_rng(0)
    B, Cc = 3, 72
    x = R.f16(rng.standard_normal((B, H, W, Cc)))
    g = G.Graph(device)
    xi = g.input((Cc, W, H, B), G.F16, "x")
    y = g.output(G.mean_2d(G.ModelRef(g), xi), "mean")
    g.allocate()
    assert g.describe().startswith(f"mean_2d [{Cc}, {W}, {H}, {B}]")
    g.set(xi, x)
    g.compute()
    first = g.get(y)
    err = float(np.abs(first - R.mean_2d(x)).max())
    print(f"mean_2d n={W * H}: max abs error {err:.3g}")
    assert first.shape == (B, 1, 1, Cc) and err < MEAN_BOUND
    for _ in range(5):  # a fixed summation order: the same bits every launch
        g.compute()
        np.testing.assert_array_equal(g.get(y), first)
    out, xd = empty(B * Cc * 2, zero=False), dev(x.astype(np.float16))
    for _ in range(5):
        L.vx_check(api().vx_mean_2d_f16(xd.ptr, out.ptr, B, W * H, Cc, None))
        sync()
        np.testing.assert_array_equal(out.to_numpy(np.float16, (B, 1, 1, Cc)).astype(np.float32), first)


@pytest.mark.parametrize("src,dst", [((1, 1), (6, 4)), ((12, 8), (3, 2))])  # (W, H): a 1 x 1 source (aspp_deformable's x5); a smaller target
def test_bilinear_align_corners_from_one_pixel_and_downwards(device, src, dst):
    rng = np.random.default_rng(src[0])
    B, Cc = 2, 16
    x = R.f16(rng.standard_normal((B, src[1], src[0], Cc)))
    g = G.Graph(device)
    xi = g.input((Cc, src[0], src[1], B), G.F16, "x")
    y = g.output(G.interpolate(G.ModelRef(g), xi, dst, G.BILINEAR_AC), "y")
    g.allocate()
    g.set(xi, x)
    g.compute()
    err = rel_err(g.get(y), R.bilinear_ac(x, dst[1], dst[0]))
    print(f"bilinear_ac {src} -> {dst}: rel_err {err:.3g}")
    assert g.get(y).shape == (B, dst[1], dst[0], Cc) and err < INTERPOLATE_BOUND


# ---- basic_decoder_block against the oracle's squeeze block ----------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def squeeze():
    """test_birefnet_every_level's setup: SWIN_MINI at image_size 256, seed 6, one 192 x 128 image; the oracle's feature_3 and squeeze captures."""
    cfg = dataclasses.replace(synth.SWIN_MINI, image_size=256)
    sd = synth.birefnet_state_dict(cfg, 6)
    tensors, conv_idx = synth.birefnet_gguf_tensors(sd)
    om = oracle.Model(tensors, conv_idx)
    P = oracle.swin_params(cfg.embed_dim, cfg.window_size, cfg.depths, cfg.n_heads)
    img = synth.images(1, 192, 128, seed=21)[0]
    pre = ((img.astype(np.float32) / 255.0 - np.array([0.485, 0.456, 0.406], np.float32)) / np.array([0.229, 0.224, 0.225], np.float32)).astype(np.float32)
    _, caps = oracle.birefnet_predict(om, P, pre, captures={"feature_3": 4 * 6 * 960, "squeeze": 4 * 6 * 512})
    block = {k: R.f16(v) for k, v in sd.items() if k.startswith("squeeze_module.0.")}  # what the oracle reads: the f16 tensors of the file
    x = R.f16(caps["feature_3"].reshape(1, 4, 6, 960))
    return block, x, caps["squeeze"].reshape(1, 4, 6, 512).astype(np.float64), R.decoder_block(block, "squeeze_module.0", x)


def _block_graph(device, block, fused, hip_graph=False):
    g = G.Graph(device)
    for name, a in block.items():
        g.add_weight(name, a.transpose(0, 2, 3, 1) if a.ndim == 4 else a, G.F16 if a.ndim == 4 else G.F32)
    xi = g.input((960, 6, 4, 1), G.F16, "feature_3")
    y = g.output(G.birefnet_basic_decoder_block(G.ModelRef(g, "squeeze_module.0"), xi), "squeeze")
    g.set_fused_models(fused)
    g.allocate()
    g.use_hip_graph(hip_graph)
    return g, xi, y


def test_decoder_block_against_the_oracle(device, squeeze):
    block, x, want_oracle, want_f64 = squeeze
    got = {}
    for fused in (True, False):
        g, xi, y = _block_graph(device, block, fused)
        lines = g.describe().splitlines()
        n_off, n_def = sum(l.startswith("deform_offsets") for l in lines), sum(l.startswith("deform_conv") for l in lines)
        assert (n_off, n_def) == ((4, 4) if fused else (0, 4)), lines
        assert sum(l.startswith("sigmoid") for l in lines) == (0 if fused else 4) and sum(l.startswith("mean_2d") for l in lines) == 1
        assert sum(l.startswith("bilinear_ac 1x1 -> 6x4") for l in lines) == 1
        g.set(xi, x)
        g.compute()
        got[fused] = g.get(y).astype(np.float64)
        e_or, e_64 = rel_err(got[fused], want_oracle), rel_err(got[fused], want_f64)
        m_or = float(np.abs(got[fused] - want_oracle).mean() / np.abs(want_oracle).max())
        print(f"decoder block fused={fused}: rel_err {e_or:.3g} / mean abs {m_or:.3g} of the largest value against the oracle; rel_err {e_64:.3g} against float64")
        assert e_or < 2e-2 and m_or < 4e-3, (fused, e_or, m_or)  # the hand schedule's bounds for this capture (test_birefnet_every_level)
        assert e_64 < 2e-2, (fused, e_64)
    print(f"oracle (f32) against float64: rel_err {rel_err(want_oracle, want_f64):.3g}")
    g, xi, y = _block_graph(device, block, True, hip_graph=True)
    g.set(xi, x)
    for _ in range(3):  # eager, then the captured hipGraph twice
        g.compute()
        np.testing.assert_array_equal(g.get(y).astype(np.float64), got[True])

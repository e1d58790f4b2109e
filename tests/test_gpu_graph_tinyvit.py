"""-m gpu: the graph layer's depthwise conv (csrc/kernels_dwconv.hip), the 3-channel image in front of a first conv (image_pad8), the packed-bias
window attention on the q|k|v product's rows, and the TinyViT encoder built through vision.cpp_amd/graph.py::tinyvit_encode -- against float64 numpy on
f16-rounded operands (tests/dwconv_ref.py) and against the CPU oracle's restatement of src/visp/arch/mobile-sam.cpp, stage by stage.

Depthwise bound: the floor of the comparison is the float64 result rounded to f16 against itself; the kernel adds f32 roundings of at most 49 products
(49 x 2^-24 = 3e-6 of a value) and, with GELU, v_exp / v_rcp at one ulp of f32 -- far below one f16 rounding --, so the bound is 4 x the floor (the rule
of DESIGN.md section 14). Measured on MI355X, per case of DW_CASES, the error equals the floor to three digits (direct launch and through the graph alike):
  (8,5,7,2,3,1,1,none) 2.46e-4    (72,9,13,2,3,2,1,gelu) 2.84e-4    (16,6,6,1,4,1,2,none) 2.92e-4    (16,8,10,2,4,2,1,leaky) 2.27e-4
  (24,7,11,1,5,1,2,none) 2.59e-4  (8,4,6,1,7,1,3,gelu) 2.63e-4      (64,3,3,1,1,1,0,none) 2.62e-4    (40,2,19,3,3,1,1,none) 2.31e-4
Window attention on the q|k|v rows (norm, q|k|v, attention, projection) against float64, of the largest output: 4.9e-4 / 7.2e-4 / 6.5e-4 fused, 4.9e-4 /
6.8e-4 / 6.3e-4 per node, 4.4e-4 / 7.9e-4 / 5.2e-4 between the two, at (heads, T, windows) = (1, 49, 6), (3, 196, 2), (10, 49, 3); bound 4e-3.
tinyvit_encode of TINYVIT_MINI against the oracle: mean errors 9e-5 .. 4.4e-4 per stage and 6.7e-4 at the output (bounds 6e-3), largest 4.3e-3 at patch_embed
(bound 0.08 x 8.75) and 4.4e-3 at the output (bound 0.1), fused and per node alike."""

import numpy as np
import pytest

import dwconv_ref as R
from oracle import oracle
from visioncpp_amd import _lib as L
from visioncpp_amd import graph as G
from visioncpp_amd import synth, vision

pytestmark = pytest.mark.gpu

from gpu_util import api, dev, empty, release, sync  # noqa: E402


@pytest.fixture(scope="module")
def device():
    assert api().vx_device_count() > 0, "no HIP device visible: the product path has no CPU fallback"
    return vision.Device.init(vision.Backend.gpu)


@pytest.fixture(autouse=True)
def _release_buffers():
    yield
    release()


# ---- vx_dwconv_f16 ------------------------------------------------------------------------------------------------------------------------------

# (C, H, W, B, k, stride, pad, act): C below, at and across the 8 channel groups a wave's lanes run over first; strips with tails (W = 7, 13, 19 against
# 8 and 4 outputs per thread); maps smaller than the kernel (4 x 6 under 7x7, 3 x 3 under 1x1 / 2 x 19 under 3x3); even kernels; both strides
DW_CASES = [(8, 5, 7, 2, 3, 1, 1, "none"), (72, 9, 13, 2, 3, 2, 1, "gelu"), (16, 6, 6, 1, 4, 1, 2, "none"), (16, 8, 10, 2, 4, 2, 1, "leaky"),
            (24, 7, 11, 1, 5, 1, 2, "none"), (8, 4, 6, 1, 7, 1, 3, "gelu"), (64, 3, 3, 1, 1, 1, 0, "none"), (40, 2, 19, 3, 3, 1, 1, "none")]
SLOPE = 0.2
_dw_cache = {}


def _dw_case(i):
    """operands as f16 values and the float64 result, computed once per case and shared by the direct and the graph test; odd cases carry no bias,
    cases 2, 3, 6, 7 use the [1, kw, kh, C] stored form"""
    if i not in _dw_cache:
        Cc, H, W, B, k, s, pad, act = DW_CASES[i]
        rng = np.random.default_rng(100 + i)
        x = R.f16(rng.standard_normal((B, H, W, Cc)))
        w = R.f16(rng.standard_normal((k, k, Cc)) / k)
        b = None if i % 2 else (rng.standard_normal(Cc) * 0.3).astype(np.float32)
        y = R.depthwise_conv2d(x, w, b, s, pad)
        want = R.gelu_tanh(y) if act == "gelu" else (R.leaky_relu(y, np.float32(SLOPE)) if act == "leaky" else y)
        for a in (x, w, want):
            a.setflags(write=False)
        _dw_cache[i] = (x, w, b, want, R.f16_floor(want))
    return _dw_cache[i]


@pytest.mark.parametrize("i", range(len(DW_CASES)))
def test_dwconv_launcher_against_float64(i):
    Cc, H, W, B, k, s, pad, act = DW_CASES[i]
    x, w, b, want, floor = _dw_case(i)
    out = empty(want.size * 2, zero=False)
    bd = dev(b) if b is not None else None
    L.vx_check(api().vx_dwconv_f16(dev(x.astype(np.float16)).ptr, dev(w.astype(np.float16).reshape(k * k, Cc)).ptr, bd.ptr if bd else None, out.ptr, B, H, W, Cc, k, s, pad,
                                   {"none": 0, "gelu": 1, "leaky": 2}[act], SLOPE, None))
    sync()
    got = out.to_numpy(np.float16, want.shape)
    err = R.rel_err(got, want)
    print(f"dwconv {DW_CASES[i]}: rel err {err:.3g} floor {floor:.3g} bound {4 * floor:.3g}")
    assert np.isfinite(got.astype(np.float32)).all() and err <= 4 * floor, (DW_CASES[i], err, floor)


def test_dwconv_launcher_refuses_what_it_was_not_built_for():
    x = dev(np.zeros((1, 4, 4, 8), np.float16))
    y = empty(4 * 4 * 8 * 2)
    for args, msg in [((1, 4, 4, 12, 3, 1, 1, 0), b"multiple of 8"), ((1, 4, 4, 8, 8, 1, 1, 0), b"kernel 8"), ((1, 4, 4, 8, 3, 3, 1, 0), b"stride 3"),
                      ((1, 4, 4, 8, 3, 1, 3, 0), b"pad 3"), ((1, 4, 4, 8, 7, 1, 0, 0), b"does not fit"), ((1, 4, 4, 8, 3, 1, 1, 3), b"activation 3")]:
        assert api().vx_dwconv_f16(x.ptr, x.ptr, None, y.ptr, *args, 0.0, None) == 0 and msg in api().vx_last_error(), msg


@pytest.mark.parametrize("i", range(len(DW_CASES)))
def test_dwconv_node_against_float64(device, i):
    Cc, H, W, B, k, s, pad, act = DW_CASES[i]
    x, w, b, want, floor = _dw_case(i)
    g = G.Graph(device)
    g.add_weight("dw.weight", R.kernel_forms(w)[(i // 2) % 2].astype(np.float32), G.F16)
    if b is not None:
        g.add_weight("dw.bias", b, G.F32)
    m = G.ModelRef(g, "dw")
    xi = g.input((Cc, W, H, B), G.F16, "x")
    y = G.conv_2d_depthwise(m, xi, s, pad)
    y = G.gelu(m, y) if act == "gelu" else (G.leaky_relu(m, y, SLOPE) if act == "leaky" else y)
    g.output(y, "y")
    g.allocate()
    lines = g.describe().strip().splitlines()[:-1]
    tag = {"none": "", "gelu": "[gelu]", "leaky": "[leaky_relu]"}[act]
    assert len(lines) == 1 and lines[0].startswith(f"dwconv{k}x{k}{'s2' if s == 2 else ''}{tag} "), lines
    g.set(xi, x)
    g.compute()
    got = g.get(y)
    assert got.shape == want.shape
    err = R.rel_err(got, want)
    print(f"dwconv node {DW_CASES[i]}: rel err {err:.3g} floor {floor:.3g}")
    assert err <= 4 * floor, (DW_CASES[i], err, floor)


# ---- image_pad8 + the first conv --------------------------------------------------------------------------------------------------------------

def test_image_pad8_pixels_are_value_residue_zero():
    rng = np.random.default_rng(5)
    img = np.concatenate([rng.standard_normal(3 * 331) * 1.5, [0.0, 1.0, -2.6401, 1e-3, 255.0, 0.1]]).astype(np.float32)
    n = img.size // 3
    out = empty(n * 16, zero=False)
    L.vx_check(api().vx_image_pad8_f32(dev(img).ptr, out.ptr, n, None))
    sync()
    got = out.to_numpy(np.float16, (n, 8))
    v = img.reshape(n, 3)
    hi = v.astype(np.float16)
    np.testing.assert_array_equal(got[:, 0:3], hi)
    np.testing.assert_array_equal(got[:, 3:6], (v - hi.astype(np.float32)).astype(np.float16))
    assert not got[:, 6:8].any()
    # value + residue give the f32 pixel back up to the residue's own rounding (2^-11 of at most 2^-11 |v|; 2^-25 once the residue is an f16 subnormal)
    back = got[:, 0:3].astype(np.float64) + got[:, 3:6].astype(np.float64)
    assert (np.abs(back - v) <= np.maximum(2.0 ** -22 * np.abs(v), 2.0 ** -24)).all()
    assert api().vx_image_pad8_f32(None, out.ptr, n, None) == 0 and b"vx_image_pad8_f32" in api().vx_last_error()


def test_first_conv_on_the_f32_image_beats_the_f16_rounded_image(device):
    """conv 3x3 stride 2, 3 -> 16 channels, on a 10 x 14 image of normalised pixels, against float64 on the UNROUNDED f32 image. Both runs round their
    output to f16; the run on the f16-rounded image (the same conv GEMM on 8-channel pixels whose channels 3..7 are zero) adds the image's rounding to
    that, of comparable size (27 taps x 2^-12 |x| |w| against 2^-12 |y|), so its RMS error must be the larger one. Measured on MI355X: RMS error
    3.75e-4 with the residue lanes, 5.23e-4 on the rounded image (max 1.93e-3 against 2.29e-3; outputs up to 8)."""
    rng = np.random.default_rng(11)
    B, H, W, Co = 2, 10, 14, 16
    img = ((rng.random((B, H, W, 3)) - np.array([0.485, 0.456, 0.406])) / np.array([0.229, 0.224, 0.225])).astype(np.float32)
    w = R.f16(rng.standard_normal((Co, 3, 3, 3)) * 1.5 / np.sqrt(27.0))
    b = (rng.standard_normal(Co) * 0.1).astype(np.float32)
    want = R.conv2d(img.astype(np.float64), w, b, 2, 1)

    g = G.Graph(device)
    g.add_weight("c.weight", w.astype(np.float32), G.F16)
    g.add_weight("c.bias", b, G.F32)
    w8 = np.zeros((Co, 3, 3, 8), np.float32)
    w8[..., :3] = w
    g.add_weight("c8.weight", w8, G.F16)
    g.add_weight("c8.bias", b, G.F32)
    xi = g.input((3, W, H, B), G.F32, "image")
    x8 = g.input((8, W, H, B), G.F16, "image_f16")
    ya = g.output(G.conv_2d(G.ModelRef(g, "c"), xi, 2, 1), "on_f32")
    yb = g.output(G.conv_2d(G.ModelRef(g, "c8"), x8, 2, 1), "on_f16")
    g.allocate()
    lines = g.describe().strip().splitlines()[:-1]
    assert lines == ["image_pad8 [3, 14, 10, 2]", "conv3x3s2 M=70 N=16 K=72 <- c.weight", "conv3x3s2 M=70 N=16 K=72 <- c8.weight"], lines
    g.set(xi, img)
    rounded = np.zeros((B, H, W, 8), np.float16)
    rounded[..., :3] = img.astype(np.float16)
    g.set(x8, rounded)
    g.compute()
    ea, eb = g.get(ya) - want, g.get(yb) - want
    rms_a, rms_b = float(np.sqrt((ea ** 2).mean())), float(np.sqrt((eb ** 2).mean()))
    print(f"first conv: rms error {rms_a:.3g} (max {np.abs(ea).max():.3g}) with residue lanes, {rms_b:.3g} (max {np.abs(eb).max():.3g}) on the f16-rounded image")
    assert R.rel_err(g.get(ya), want) < 1e-3  # two f16 roundings of the largest value at most
    assert rms_a < rms_b, (rms_a, rms_b)


def test_pointwise_conv_on_the_f32_image_takes_the_same_path(device):
    """A 1x1 conv on the f32 image must not read it as f16 rows: it goes through image_pad8 and the conv loader like any other kernel. Bound: two f16
    roundings (2^-11 each) of the largest output."""
    rng = np.random.default_rng(12)
    B, H, W, Co = 1, 5, 9, 8
    img = (rng.standard_normal((B, H, W, 3)) * 1.5).astype(np.float32)
    w = R.f16(rng.standard_normal((Co, 1, 1, 3)))
    g = G.Graph(device)
    g.add_weight("p.weight", w.astype(np.float32), G.F16)
    xi = g.input((3, W, H, B), G.F32, "image")
    y = g.output(G.conv_2d(G.ModelRef(g, "p"), xi), "y")
    g.allocate()
    assert g.describe().strip().splitlines()[:-1] == ["image_pad8 [3, 9, 5, 1]", "conv1x1 M=45 N=8 K=8 <- p.weight"]
    g.set(xi, img)
    g.compute()
    assert R.rel_err(g.get(y), R.conv2d(img.astype(np.float64), w)) < 2.0 ** -10


# ---- the packed-bias window attention ------------------------------------------------------------------------------------------------------------

ATTN_BOUND = 4e-3  # of the largest output: the bound of the masked attention's own tests


@pytest.mark.parametrize("heads,T,windows", [(1, 49, 6), (3, 196, 2), (10, 49, 3)])
def test_window_attention_on_the_qkv_rows_against_per_node_and_float64(device, heads, T, windows):
    dim = 32 * heads
    rng = np.random.default_rng(heads * T)
    p = {"norm.weight": (1 + 0.05 * rng.standard_normal(dim)).astype(np.float32), "norm.bias": (0.05 * rng.standard_normal(dim)).astype(np.float32),
         "qkv.weight": R.f16(rng.standard_normal((3 * dim, dim)) / np.sqrt(dim)), "qkv.bias": (0.02 * rng.standard_normal(3 * dim)).astype(np.float32),
         "attention_biases_indexed": R.f16(0.5 * rng.standard_normal((heads, T, T))),
         "proj.weight": R.f16(rng.standard_normal((dim, dim)) * 0.4 / np.sqrt(dim)), "proj.bias": (0.02 * rng.standard_normal(dim)).astype(np.float32)}
    x = R.f16(rng.standard_normal((windows, T, dim)))
    want = R.attention_rel_bias(p, x, heads)
    got = {}
    for fused in (True, False):
        g = G.Graph(device)
        for name, a in p.items():
            g.add_weight(f"attn.{name}", np.asarray(a, np.float32), G.F16 if a.dtype == np.float64 else G.F32)
        xi = g.input((dim, T, windows), G.F16, "x")
        out = g.output(G.tinyvit_attention_rel_bias(G.ModelRef(g, "attn"), xi, dim, heads), "out")
        g.set_fused_models(fused)
        g.allocate()
        lines = g.describe().strip().splitlines()[:-1]
        if fused:
            assert sum(l.startswith("window_attention") for l in lines) == 1 and not [l for l in lines if l.startswith(("heads_major", "attention_masked", "permute", "slice"))], lines
        else:
            assert sum(l.startswith("attention_masked") for l in lines) == 1 and sum(l.startswith("heads_major") for l in lines) == 3, lines
        g.set(xi, x)
        g.compute()
        got[fused] = g.get(out).reshape(want.shape)
        assert np.isfinite(got[fused]).all()
    e_f, e_n, e_fn = R.rel_err(got[True], want), R.rel_err(got[False], want), R.rel_err(got[True], got[False])
    print(f"window attention heads={heads} T={T}: fused {e_f:.3g}, per node {e_n:.3g}, fused vs per node {e_fn:.3g}; bound {ATTN_BOUND}")
    assert e_f < ATTN_BOUND and e_n < ATTN_BOUND and e_fn < ATTN_BOUND, (e_f, e_n, e_fn)


# ---- the TinyViT encoder through the graph layer -----------------------------------------------------------------------------------------------

MEAN, STD = np.array([0.485, 0.456, 0.406], np.float32), np.array([0.229, 0.224, 0.225], np.float32)
STAGES = ["patch_embed", "layer_0", "layer_1", "layer_2", "layer_3"]


@pytest.fixture(scope="module")
def mini(tmp_path_factory):
    """the mini encoder's file, two normalised images, and the oracle's stages for each (computed once, read-only)"""
    cfg = synth.TINYVIT_MINI
    sd = synth.tinyvit_state_dict(cfg, 3)
    path = synth.write_tinyvit_gguf(tmp_path_factory.mktemp("tinyvit") / "mini.gguf", cfg, sd=sd)
    tensors, conv2d = synth.tinyvit_gguf_tensors(sd)
    om = oracle.Model(tensors, conv2d, "whcn")
    layers = cfg.layers()
    pre = ((synth.images(2, cfg.img_size, cfg.img_size, seed=21).astype(np.float32) / np.float32(255.0) - MEAN) / STD).astype(np.float32)
    sizes = {"patch_embed": (cfg.img_size // 4) ** 2 * cfg.embed_dims[0], **{f"layer_{k}": layers[min(k + 1, 3)][0] ** 2 * layers[min(k + 1, 3)][1] for k in range(4)}}
    want = [oracle.tinyvit_encode(om, oracle.tinyvit_params(cfg.img_size, layers), pre[i], captures=sizes) for i in range(2)]
    for y, caps in want:
        y.setflags(write=False)
    return dict(cfg=cfg, path=path, pre=pre, want=want)


def _encoder(device, mini, fused, batch):
    cfg = mini["cfg"]
    g = G.Graph(device, G.Weights(mini["path"]))
    image = g.input((3, cfg.img_size, cfg.img_size, batch), G.F32, "image")
    out = g.output(G.tinyvit_encode(G.ModelRef(g, "enc"), image, cfg.layers()), "out")
    names = {"patch_embed": "enc.patch_embed", **{f"layer_{k}": f"enc.layers.{k}" for k in range(4)}}
    stages = {k: g.output(g.get_tensor(n), k) for k, n in names.items()}
    g.set_fused_models(fused)
    g.use_hip_graph(True)
    g.allocate()
    return g, image, out, stages


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "per_node"])
def test_tinyvit_encode_every_stage_against_the_oracle(device, mini, fused):
    """The bounds of tests/test_gpu_tinyvit.py for the hand schedule: f16 storage of the chained maps against the f32 oracle, per stage."""
    g, image, out, stages = _encoder(device, mini, fused, 2)
    lines = g.describe().strip().splitlines()[:-1]
    assert sum(l.startswith("window_attention" if fused else "attention_masked") for l in lines) == 4 and lines[0].startswith("image_pad8")
    g.set(image, mini["pre"])
    g.compute()
    got = g.get(out)  # [B, H, W, 256]
    got_stages = {k: g.get(t).reshape(2, -1) for k, t in stages.items()}
    for i in range(2):
        y, caps = mini["want"][i]
        for k in STAGES:
            want = caps[k]
            assert got_stages[k][i].shape == want.shape, k
            err = np.abs(got_stages[k][i] - want)
            scale = np.abs(want).mean()
            print(f"{'fused' if fused else 'per node'} image {i} {k}: mean err {err.mean():.3g} max {err.max():.3g} (scale {scale:.3g}, max {np.abs(want).max():.3g})")
            assert err.mean() < 6e-3 * max(1.0, scale) and err.max() < 0.08 * max(1.0, np.abs(want).max()), (k, err.mean(), err.max(), scale)
        err = np.abs(got[i] - y)
        print(f"{'fused' if fused else 'per node'} image {i} output: mean err {err.mean():.3g} max {err.max():.3g}")
        assert err.mean() < 6e-3 and err.max() < 0.1, (err.mean(), err.max())
    # the second compute replays the launch list as one hipGraph: bit-identical
    g.compute()
    np.testing.assert_array_equal(g.get(out), got)
    for k, t in stages.items():
        np.testing.assert_array_equal(g.get(t).reshape(2, -1), got_stages[k])
    # an image encoded alone gives the bits it gives as part of the batch
    g1, image1, out1, _ = _encoder(device, mini, fused, 1)
    for i in range(2):
        g1.set(image1, mini["pre"][i:i + 1])
        g1.compute()
        np.testing.assert_array_equal(g1.get(out1)[0], got[i])

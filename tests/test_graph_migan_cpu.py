"""The graph layer's clamp op, plane broadcast, 4-channel image conv and the MI-GAN builders without a GPU (`Graph(None)`): shape inference, host folding,
every refusal by its message, the planned launch lists of migan_generate at res 32 with fused models and per node (ch_base = 256, ch_max = 24: level widths
8, 16, 24, 24, none a multiple of 64, which the hand schedule of csrc/migan.cpp refuses), the group that must NOT fuse (a filter_const that is not the
zero-insertion tile), the C++ face (tests/cpp/migan_graph_check.cpp) against the Python face, and the lowering fingerprints of every model that existed
before, which must not move."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import fir_ref as R
from visioncpp_amd import _lib as L
from visioncpp_amd import graph as G
from visioncpp_amd import synth

ROOT = Path(__file__).resolve().parents[1]
RES, CH = 32, dict(ch_base=256, ch_max=24)


@pytest.fixture(scope="module")
def gguf(tmp_path_factory):
    return synth.write_migan_gguf(tmp_path_factory.mktemp("migan") / "migan32.gguf", RES, seed=1, **CH)


def _lines(g):
    return g.describe().strip().splitlines()[:-1]


def _generate(path, fused, batch=2):
    g = G.Graph(None, G.Weights(path))
    g.set_fused_models(fused)
    out = G.migan_generate(G.ModelRef(g), g.input((4, RES, RES, batch), G.F32, "image"), RES)
    g.allocate()
    return g, out


# ---- clamp ---------------------------------------------------------------------------------------------------------------------------------------

def test_clamp_shape_and_host_folding():
    assert G.OP_CLAMP == 37
    g = G.Graph(None)
    m = G.ModelRef(g)
    x = g.input((16, 5, 3, 2), G.F16, "x")
    y = G.clamp(m, x, -256.0, 256.0)
    assert y.ne == x.ne and y.dtype == G.F16 and not y.is_constant
    v = np.array([60000.0, -60000.0, 256.0, -256.0, 255.9, -255.9, 0.0, -0.0], np.float32)
    c = G.clamp(m, g.add_weight("c", v, G.F32), -256.0, 256.0)
    assert c.is_constant
    got = g.read_constant(c).ravel()
    np.testing.assert_array_equal(got, R.clamp(v, -256.0, 256.0).astype(np.float32))
    assert np.signbit(got[7]) and not np.signbit(got[6])  # -0.0 stays -0.0


def test_clamp_refusals():
    g = G.Graph(None)
    m = G.ModelRef(g)
    x = g.input((16, 5, 3, 2), G.F16, "x")
    with pytest.raises(L.Error, match="clamp: lower bound 2 above upper bound 1"):
        G.clamp(m, x, 2.0, 1.0)
    for lo, hi in ((-np.inf, 1.0), (0.0, np.inf), (np.nan, 1.0)):
        with pytest.raises(L.Error, match="clamp: bounds .* both must be finite"):
            G.clamp(m, x, lo, hi)
    with pytest.raises(L.Error, match="clamp: operand 0 is f32"):
        G.clamp(m, g.input((16, 5, 3, 2), G.F32, "xf"), -1.0, 1.0)
    with pytest.raises(L.Error, match="clamp: two float parameters"):
        g.op(G.OP_CLAMP, [x], fparams=[1.0])


# ---- plane broadcast ---------------------------------------------------------------------------------------------------------------------------------

def test_plane_broadcast_is_accepted_and_folded():
    g = G.Graph(None)
    m = G.ModelRef(g)
    x = g.input((16, 5, 3, 2), G.F16, "x")
    for dtype, name in ((G.F16, "p16"), (G.F32, "p32")):
        p = g.add_weight(name, np.arange(15, dtype=np.float32).reshape(1, 3, 5, 1), dtype)
        assert p.ne == (1, 5, 3, 1)
        for fn in (G.add, G.mul, G.sub):
            assert fn(m, x, p).ne == x.ne
    assert G.mul(m, x, g.input((1, 5, 3, 1), G.F16, "pa")).ne == x.ne  # an activation
    # on constants: folded with the pixel's value for every channel and image
    a = np.random.default_rng(0).standard_normal((2, 3, 5, 16)).astype(np.float32)
    b = np.random.default_rng(1).standard_normal((3, 5)).astype(np.float32)
    ca, cb = g.add_weight("ca", a, G.F32), g.add_weight("cb", b.reshape(1, 3, 5, 1), G.F32)
    for fn, op in ((G.add, R.ADD), (G.mul, R.MUL), (G.sub, R.SUB)):
        t = fn(m, ca, cb)
        assert t.is_constant
        np.testing.assert_array_equal(g.read_constant(t), R.plane_binary(op, a.astype(np.float64), b.astype(np.float64)).astype(np.float32))
    # noise_const * noise_strength (migan.cpp:71-72): the trailing rule, folded as before
    nz = G.mul(m, g.add_weight("nc", b, G.F32), g.add_weight("ns", np.array([0.5], np.float32), G.F32))
    np.testing.assert_array_equal(g.read_constant(nz), b[None, None] * 0.5)


def test_plane_broadcast_refusals_name_both_forms():
    g = G.Graph(None)
    m = G.ModelRef(g)
    x = g.input((16, 5, 3, 2), G.F16, "x")
    both = r"must equal the first in its leading dimensions and be 1 in the rest, or be a plane \[1, W, H, 1\] on \[C, W, H, N\]"
    for shape in ((1, 5, 1, 1), (1, 5, 3, 2), (1, 4, 3, 1)):
        for fn, name in ((G.add, "add"), (G.mul, "mul"), (G.sub, "sub")):
            with pytest.raises(L.Error, match=rf"{name}: cannot broadcast .*{both}"):
                fn(m, x, g.input(shape, G.F16, f"b{shape}{name}"))


def test_plane_ops_are_one_launch_each():
    g = G.Graph(None)
    m = G.ModelRef(g)
    x = g.input((16, 5, 3, 2), G.F16, "x")
    p = g.add_weight("p", np.ones((1, 3, 5, 1), np.float32), G.F32)
    q = g.input((1, 5, 3, 1), G.F16, "q")
    g.output(G.clamp(m, G.sub(m, G.add(m, G.mul(m, x, p), q), p), -1.0, 1.0), "y")
    g.allocate()
    assert _lines(g) == ["mul_plane B=2 HW=15 C=16 (constant)", "add_plane B=2 HW=15 C=16", "sub_plane B=2 HW=15 C=16 (constant)", "clamp n=480"]
    g = G.Graph(None)
    g.output(G.add(G.ModelRef(g), g.input((12, 5, 3, 2), G.F16, "x"), g.add_weight("p", np.ones((1, 3, 5, 1), np.float32), G.F32)), "y")
    with pytest.raises(L.Error, match=r"add: a plane operand on 12 channels \(a multiple of 8\)"):
        g.allocate()


# ---- f32 image of 4 channels -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [1, 3])
def test_four_channel_image_conv_is_accepted(k):
    g = G.Graph(None)
    m = G.ModelRef(g)
    rng = np.random.default_rng(k)
    g.add_weight("c.weight", rng.standard_normal((16, k, k, 4)).astype(np.float32), G.F16)  # [Cin, kw, kh, Cout] = [4, k, k, 16]
    g.add_weight("c.bias", rng.standard_normal(16).astype(np.float32), G.F32)
    y = G.conv_2d(m["c"], g.input((4, 9, 7, 2), G.F32, "image"), 1, k // 2)
    assert y.ne == (16, 9, 7, 2) and y.dtype == G.F16
    g.add_weight("c5.weight", np.zeros((16, 1, 1, 5), np.float32), G.F16)
    with pytest.raises(L.Error, match="conv_2d: operand 0 is f32"):  # 5 channels are not an image this layer reads
        G.conv_2d(m["c5"], g.input((5, 9, 7, 2), G.F32, "image5"), 1, 0)
    g.output(y, "y")
    g.allocate()
    lines = _lines(g)
    assert lines[0] == "image4_pad8 [4, 9, 7, 2]" and lines[1].startswith(f"conv{k}x{k} M=126 N=16 K={8 * k * k} ") and len(lines) == 2, lines  # K counts the 8-channel value | residue pixels


# ---- the generator -----------------------------------------------------------------------------------------------------------------------------------

FUSED_KINDS = ("image4_pad8 ", "dwconv3x3[lrelu_agc 0.2 1.41421 256] ", "dwconv4x4s2 ", "conv1x1 ", "gemm(conv1x1)[", "upfirdn2x")


def test_generate_fused_is_only_image_depthwise_gemm_and_upfirdn_launches(gguf):
    g, out = _generate(gguf, True)
    assert out.ne == (3, RES, RES, 2) and out.dtype == G.F16
    assert synth.migan_channels(RES, **CH) == [8, 16, 24, 24]
    lines = _lines(g)
    assert lines[-1] == "slice [8, 32, 32, 2] -> [3, 32, 32, 2]"  # the one launch of the 8-channel image path's departure
    for l in lines[:-1]:
        assert l.startswith(FUSED_KINDS), l
        assert not l.startswith(("leaky_relu", "scale", "clamp", "mul", "add", "nearest", "slice", "cont", "pad_rows")), l
    count = lambda s: sum(l.startswith(s) for l in lines)
    # 4 levels: fromrgb + 8 encoder 1x1 + 8 synthesis 1x1 + 4 torgb; 16 3x3 depthwise; 3 downsamples; 3 feature + 3 image upsamples
    assert (count("image4_pad8"), count("gemm(conv1x1)[") + count("conv1x1 "), count("dwconv3x3[lrelu_agc"), count("dwconv4x4s2"), count("upfirdn2x")) == (1, 21, 16, 3, 6), lines
    assert count("upfirdn2x[+plane][lrelu_agc 0.2 1.41421 256][+res]") == 3 and count("upfirdn2x[+res]") == 3
    assert count("gemm(conv1x1)[+plane][lrelu_agc") == 3 and count("gemm(conv1x1)[lrelu_agc 0.2 1.41421 256][+res]") == 1 and count("conv1x1 ") == 7  # (torgb, the conv in front of an upsample)
    assert len(lines) == 48


def test_generate_per_node_is_one_launch_per_op(gguf):
    g, _ = _generate(gguf, False)
    lines = _lines(g)
    count = lambda s: sum(l.startswith(s) for l in lines)
    assert not any(l.startswith("upfirdn2x") or "lrelu_agc" in l for l in lines)
    assert count("clamp n=") == count("leaky_relu n=") == count("scale n=") == 33  # fromrgb + 2 per separable conv (16)
    assert (count("nearest "), count("mul_plane "), count("dwconv4x4 "), count("add_plane ")) == (6, 6, 6, 6)
    assert count("slice ") == 7 and len(lines) == 195


def test_a_filter_const_that_is_not_the_tile_keeps_the_upsample_per_node(tmp_path):
    sd = synth.migan_state_dict(RES, seed=1, **CH)
    sd["synthesis.b16.conv1.upsample.filter_const"] = sd["synthesis.b16.conv1.upsample.filter_const"].copy()
    sd["synthesis.b16.conv1.upsample.filter_const"][0, 0, 3, 5] = 1.0
    g, _ = _generate(synth.write_migan_gguf(tmp_path / "changed.gguf", RES, sd=sd), True)
    lines = _lines(g)
    i = lines.index("nearest 8x8 -> 16x16 C=16")
    assert lines[i + 1:i + 4] == ["mul_plane B=2 HW=256 C=16 (constant)", "dwconv4x4 B=2 16x16 -> 17x17 C=16 pad=2 <- synthesis.b16.conv1.upsample.filter.weight",
                                  "slice [16, 17, 17, 2] -> [16, 16, 16, 2]"], lines[i:i + 5]
    assert sum(l.startswith("upfirdn2x") for l in lines) == 5 and sum(l.startswith("nearest") for l in lines) == 1


# ---- groups that meet, and groups next to the patterns of other lowerings ---------------------------------------------------------------------------------

def _conv_w(g, name, cin, cout, rng):
    g.add_weight(name + ".weight", rng.standard_normal((cout, 1, 1, cin)).astype(np.float32), G.F16)


def meeting_graphs(g, which):
    """graphs shared with tests/test_gpu_graph_migan.py: returns (inputs, output)"""
    m = G.ModelRef(g)
    rng = np.random.default_rng(11)
    if which == "two_agc_convs_into_one_add":
        _conv_w(g, "a", 64, 16, rng)
        _conv_w(g, "b", 64, 16, rng)
        x, y = g.input((64, 6, 4, 2), G.F16, "x"), g.input((64, 6, 4, 2), G.F16, "y")
        a = G.migan_lrelu_agc(m, G.conv_2d(m["a"], x), 0.2, G.MIGAN_SQRT2, 256)
        b = G.migan_lrelu_agc(m, G.conv_2d(m["b"], y), 0.2, G.MIGAN_SQRT2, 256)
        return [x, y], g.output(G.add(m, a, b), "o")
    if which == "two_upsamples_into_one_add":
        for n in "ab":
            g.add_weight(n + ".filter_const", np.tile(np.array([[1.0, 0.0], [0.0, 0.0]], np.float32), (4, 6))[None, None], G.F16)
            g.add_weight(n + ".filter.weight", R.perturbed_fir(rng, 8).transpose(2, 0, 1)[..., None], G.F16)
        x, y = g.input((8, 6, 4, 2), G.F16, "x"), g.input((8, 6, 4, 2), G.F16, "y")
        return [x, y], g.output(G.add(m, G.migan_upsample_2d(m["a"], x), G.migan_upsample_2d(m["b"], y)), "o")
    if which in ("silu_shortcut_add_of_an_agc_conv", "silu_shortcut_add_of_an_upsample"):  # the add is the SiLU launch's (lower_yolo.cpp), the chain its residual
        _conv_w(g, "b", 64, 16, rng)
        y = g.input((64, 12, 8, 2), G.F16, "y")
        if which == "silu_shortcut_add_of_an_agc_conv":
            _conv_w(g, "a", 64, 16, rng)
            x = g.input((64, 12, 8, 2), G.F16, "x")
            a = G.migan_lrelu_agc(m, G.conv_2d(m["a"], x), 0.2, G.MIGAN_SQRT2, 256)
        else:
            g.add_weight("a.filter_const", np.tile(np.array([[1.0, 0.0], [0.0, 0.0]], np.float32), (4, 6))[None, None], G.F16)
            g.add_weight("a.filter.weight", R.perturbed_fir(rng, 16).transpose(2, 0, 1)[..., None], G.F16)
            x = g.input((16, 6, 4, 2), G.F16, "x")
            a = G.migan_upsample_2d(m["a"], x)
        b = G.silu(m, G.conv_2d(m["b"], y))  # behind the chain in node order: the SiLU group takes add(b, a) as its shortcut
        return [x, y], g.output(G.add(m, b, a), "o")
    if which == "agc_conv_on_a_map_placed_in_a_concat":  # s is the last node of a SiLU launch that writes into the concat's buffer: the conv behind it reads it there
        _conv_w(g, "b", 64, 16, rng)
        _conv_w(g, "c", 16, 16, rng)
        y, r, other = g.input((64, 6, 4, 2), G.F16, "y"), g.input((16, 6, 4, 2), G.F16, "r"), g.input((16, 6, 4, 2), G.F16, "other")
        sm = G.add(m, G.silu(m, G.conv_2d(m["b"], y)), r)
        cat = g.output(G.concat(m, [sm, G.scale(m, other, 2.0)], 0), "cat")
        return [y, r, other], g.output(G.migan_lrelu_agc(m, G.conv_2d(m["c"], sm), 0.2, G.MIGAN_SQRT2, 256), "o")
    if which in ("agc_conv_on_a_clamped_map", "agc_conv_on_an_unbounded_map"):  # 16-wide rows are read in place only where the graph proves them finite
        g.add_weight("dw.weight", (rng.standard_normal((16, 3, 3, 1)) / 3).astype(np.float32), G.F16)
        _conv_w(g, "c", 16, 16, rng)
        x = g.input((16, 6, 4, 2), G.F16, "x")
        t = G.conv_2d_depthwise(m["dw"], x, 1, 1)
        t = G.migan_lrelu_agc(m, t, 0.2, G.MIGAN_SQRT2, 256 if which == "agc_conv_on_a_clamped_map" else 0)
        return [x], g.output(G.migan_lrelu_agc(m, G.conv_2d(m["c"], t), 0.2, G.MIGAN_SQRT2, 256), "o")
    # ops that existed before clamp did: depthwise -> leaky_relu(0.1) -> scale(2) -> conv1x1 -> concat with another map | relu
    g.add_weight("dw.weight", (rng.standard_normal((16, 3, 3, 1)) / 3).astype(np.float32), G.F16)
    _conv_w(g, "c", 16, 16, rng)
    x, other = g.input((16, 6, 4, 2), G.F16, "x"), g.input((16, 6, 4, 2), G.F16, "other")
    t = G.conv_2d(m["c"], G.scale(m, G.leaky_relu(m, G.conv_2d_depthwise(m["dw"], x, 1, 1), 0.1), 2.0))
    if which == "conv_into_concat":
        return [x, other], g.output(G.concat(m, [t, G.scale(m, other, 2.0)], 0), "o")
    return [x], g.output(G.relu(m, t), "o")


def _meeting(which, fused):
    g = G.Graph(None)
    g.set_fused_models(fused)
    meeting_graphs(g, which)
    g.allocate()
    return _lines(g)


def test_two_chains_that_meet_in_one_add_both_run():
    """the first chain takes the add with the second's last map as its residual; the second ends in front of it and is emitted first"""
    agc = "[lrelu_agc 0.2 1.41421 256]"
    assert _meeting("two_agc_convs_into_one_add", True) == [f"gemm(conv1x1){agc} M=48 N=16 K=64 <- b.weight", f"gemm(conv1x1){agc}[+res] M=48 N=16 K=64 <- a.weight"]
    assert _meeting("two_upsamples_into_one_add", True) == ["upfirdn2x B=2 6x4 -> 12x8 C=8 <- b.filter.weight", "upfirdn2x[+res] B=2 6x4 -> 12x8 C=8 <- a.filter.weight"]
    assert len(_meeting("two_agc_convs_into_one_add", False)) == 9 and len(_meeting("two_upsamples_into_one_add", False)) == 9


MEETING = ["two_agc_convs_into_one_add", "two_upsamples_into_one_add", "silu_shortcut_add_of_an_agc_conv", "silu_shortcut_add_of_an_upsample",
           "agc_conv_on_a_map_placed_in_a_concat", "agc_conv_on_a_clamped_map", "agc_conv_on_an_unbounded_map", "conv_into_concat", "conv_into_relu"]


def test_every_meeting_graph_plans_in_both_modes():
    for which in MEETING:
        for fused in (True, False):
            assert _meeting(which, fused), (which, fused)


def test_an_add_a_silu_launch_has_taken_stays_its_own():
    """the MI-GAN chain ends in front of the SiLU group's shortcut add and is that launch's residual"""
    agc = "[lrelu_agc 0.2 1.41421 256]"
    assert _meeting("silu_shortcut_add_of_an_agc_conv", True) == [f"gemm(conv1x1){agc} M=192 N=16 K=64 <- a.weight", "conv1x1[silu][+res] M=192 N=16 K=64 <- b.weight"]
    assert _meeting("silu_shortcut_add_of_an_upsample", True) == ["upfirdn2x B=2 6x4 -> 12x8 C=16 <- a.filter.weight", "conv1x1[silu][+res] M=192 N=16 K=64 <- b.weight"]
    lines = _meeting("agc_conv_on_a_map_placed_in_a_concat", True)
    assert lines[0] == "conv1x1[silu][+res][out ch 0..16 of 32] M=48 N=16 K=64 <- b.weight" and lines[-4:] == ["conv1x1[in ch 0..16 of 32] M=48 N=16 K=16 <- c.weight",
                                                                                                            "leaky_relu n=768", "scale n=768", "clamp n=768"], lines


def test_narrow_rows_are_read_in_place_only_where_the_graph_proves_them_finite():
    """0 * inf is a NaN: behind a clamp the 16-wide rows are read where they lie, behind a map without a proven bound they are copied into padded rows, as per node"""
    agc = "[lrelu_agc 0.2 1.41421 256]"
    assert _meeting("agc_conv_on_a_clamped_map", True) == [f"dwconv3x3{agc} B=2 6x4 -> 6x4 C=16 pad=1 <- dw.weight", f"gemm(conv1x1){agc} M=48 N=16 K=16 <- c.weight"]
    assert _meeting("agc_conv_on_an_unbounded_map", True) == ["dwconv3x3[lrelu_agc 0.2 1.41421 0] B=2 6x4 -> 6x4 C=16 pad=1 <- dw.weight", "pad_rows K=16->64 <- c.weight",
                                                              f"gemm(conv1x1){agc} M=48 N=16 K=16 <- c.weight"]


def test_a_conv_another_lowering_has_plans_for_is_left_to_it():
    """behind a depthwise + lrelu_agc group: a 1x1 conv that writes into its slice of a concat stays lower_yolo.cpp's, one whose relu the product takes stays gemm_like's"""
    dw = "dwconv3x3[lrelu_agc 0.1 2 0] B=2 6x4 -> 6x4 C=16 pad=1 <- dw.weight"
    assert _meeting("conv_into_concat", True) == [dw, "conv1x1[out ch 0..16 of 32] M=48 N=16 K=16 <- c.weight", "scale n=768", "concat part 1 [16, 6, 4, 2] -> [32, 6, 4, 2]"]
    assert _meeting("conv_into_relu", True) == [dw, "pad_rows K=16->64 <- c.weight", "gemm(conv1x1)[relu] M=48 N=16 K=16 <- c.weight"]
    assert _meeting("conv_into_relu", False)[-1] == "gemm(conv1x1)[relu] M=48 N=16 K=16 <- c.weight"


def test_cpp_face_plans_the_same_launches(gguf):
    """tests/cpp/migan_graph_check.cpp: separable_conv_2d in each flag combination the generator uses, and synthesis_block, through include/visp/nn.h."""
    exe = ROOT / "vision.cpp_amd" / "lib" / "migan_graph_check"
    assert exe.exists(), "built by __graft_entry__.build()"

    def plan(fused, build):
        g = G.Graph(None, G.Weights(gguf))
        g.set_fused_models(fused)
        build(g, G.ModelRef(g))
        g.allocate()
        return g.describe()

    ACT, DOWN, UP, NOISE, IMG = 1, 2, 4, 8, 16
    # (prefix, c_in, w, h, flags): the stored filter_const and noise planes are for the level's own extent, the others take any
    seps = [("encoder.b16.conv1", 16, 6, 4, ACT), ("encoder.b16.conv2", 16, 6, 4, ACT | DOWN), ("synthesis.b16.conv1", 24, 8, 8, ACT | UP | NOISE),
            ("synthesis.b16.conv2", 16, 16, 16, ACT | NOISE), ("synthesis.b4.conv1", 24, 6, 4, ACT)]
    for fused in (True, False):
        for prefix, cin, w, h, flags in seps:
            def build(g, m, prefix=prefix, cin=cin, w=w, h=h, flags=flags):
                x = g.input((cin, w, h, 2), G.F16, "x")
                g.output(G.migan_separable_conv_2d(m.with_prefix(prefix), x, bool(flags & ACT), bool(flags & DOWN), bool(flags & UP), bool(flags & NOISE)), "o0")
            r = subprocess.run([str(exe), str(gguf), "sep", prefix, str(cin), str(w), str(h), "2", str(flags), str(int(fused))], capture_output=True, text=True, timeout=120)
            assert r.returncode == 0, (r.stdout, r.stderr)
            want = plan(fused, build)
            assert r.stdout == want, (prefix, fused, r.stdout, want)

        def block(g, m):
            mb = m.with_prefix("synthesis.b16")
            x, feat, img = g.input((24, 8, 8, 2), G.F16, "x"), g.input((16, 16, 16, 2), G.F16, "feat"), g.input((8, 8, 8, 2), G.F16, "img")
            x, img = G.migan_synthesis_block(mb, x, feat, img, upsample=True, noise=True)
            g.output(img, "o1")
            g.output(x, "o0")
        r = subprocess.run([str(exe), str(gguf), "block", "synthesis.b16", "24", "8", "8", "2", str(UP | IMG), str(int(fused))], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, (r.stdout, r.stderr)
        assert r.stdout == plan(fused, block), ("block", fused, r.stdout)


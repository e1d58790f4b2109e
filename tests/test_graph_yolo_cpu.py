"""The graph layer's pooling / SiLU / softmax ops and the YOLOv9t builders without a GPU (`Graph(None)`): shape inference against tests/pool_ref.py, every
refusal by its message, the op values, the planned launch lists of the blocks with fused models (SiLU in the product's epilogue, the folded RepConv,
channel slices and concats in place, the DFL chain as one launch) and per node, the cases that must NOT fuse, the whole network at S = 96, the C++ face
(tests/cpp/yolov9t_graph_check.cpp) against the Python face, and the lowering fingerprints of every model that existed before, which must not move.

`slice` launches of the whole network: the conv network (backbone + detect convs) has none. The box decode behind it keeps three -- the class logits
read by sigmoid, and dist2bbox's two-channel lt / rb halves -- because a slice is read in place only at channel offsets that are multiples of 8 and only
by convs, pools and channel concats."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import pool_ref as R
from visioncpp_amd import _lib as L
from visioncpp_amd import graph as G
from visioncpp_amd import synth

ROOT = Path(__file__).resolve().parents[1]


@pytest.fixture(scope="module")
def gguf(tmp_path_factory):
    return synth.write_yolov9t_gguf(tmp_path_factory.mktemp("yolo") / "yolov9t.gguf", seed=1)


def _lines(g):
    return g.describe().strip().splitlines()[:-1]


def _plan(gguf, build, fused=True):
    g = G.Graph(None, G.Weights(gguf) if gguf else None)
    g.set_fused_models(fused)
    for i, t in enumerate(build(g, G.ModelRef(g))):
        g.output(t, f"o{i}")
    g.allocate()
    return g


def _x(g, c, w=12, h=9, n=2, name="x"):
    return g.input((c, w, h, n), G.F16, name)


# ---- ops -----------------------------------------------------------------------------------------------------------------------------------------

def test_op_values():
    assert (G.OP_SILU, G.OP_POOL_2D, G.OP_SOFT_MAX, G.OP_SUM_ROWS, G.OP_SUB) == (32, 33, 34, 35, 36)
    assert (G.POOL_MAX, G.POOL_AVG) == (0, 1)


@pytest.mark.parametrize("i", range(len(R.POOL_CASES)))
def test_pool_shape_inference_follows_the_reference(i):
    kind, k, s, pad, C, H, W, B = R.POOL_CASES[i]
    g = G.Graph(None)
    t = G.pool_2d(G.ModelRef(g), g.input((C, W, H, B), G.F16, "x"), kind, k, k, s, s, pad, pad)
    assert t.ne == R.pool2d(np.zeros((B, H, W, C)), kind, k, s, pad).shape[::-1] and t.dtype == G.F16 and not t.is_constant


def test_shapes_and_host_folding_of_the_other_ops():
    g = G.Graph(None)
    m = G.ModelRef(g)
    x = g.input((16, 4, 37, 2), G.F16, "x")
    assert G.silu(m, x).ne == x.ne and G.soft_max(m, x).ne == x.ne and G.sum_rows(m, x).ne == (1, 4, 37, 2)
    assert G.sub(m, x, g.input((16, 4, 1, 1), G.F16, "b")).ne == x.ne
    assert G.upscale(m, x, 2, G.SCALE_MODE_NEAREST).ne == (16, 8, 74, 2)
    v = np.array([-20.0, -0.0, 0.5, 11.0, 60000.0], np.float32)
    c = g.add_weight("c", v, G.F32)
    s = G.silu(m, c)
    assert s.is_constant
    np.testing.assert_allclose(g.read_constant(s).ravel(), R.silu(v), rtol=1e-6)
    d = G.sub(m, c, g.add_weight("one", np.ones(1, np.float32), G.F32))
    assert d.is_constant
    np.testing.assert_array_equal(g.read_constant(d).ravel(), v - 1)


def test_refusals_name_the_op():
    g = G.Graph(None)
    m = G.ModelRef(g)
    x = g.input((16, 9, 7, 2), G.F16, "x")
    for args, msg in [((G.POOL_MAX, 3, 2, 1, 1, 1, 1), "pool_2d: kernel 3x2; square kernels only"),
                      ((G.POOL_MAX, 3, 3, 1, 2, 1, 1), "pool_2d: strides 1 and 2; equal strides only"),
                      ((G.POOL_MAX, 3, 3, 3, 3, 1, 1), "pool_2d: stride 3 is not built"),
                      ((G.POOL_MAX, 14, 14, 1, 1, 7, 7), "pool_2d: kernel 14x14; kernels 1x1 up to 13x13"),
                      ((G.POOL_MAX, 3, 3, 1, 1, 2, 2), r"pool_2d: pad 2, 2 with a 3x3 kernel \(equal, 0 \.\. k / 2\)"),
                      ((G.POOL_AVG, 3, 3, 1, 1, 1, 1), "pool_2d: average pooling with pad 1 is not built"),
                      ((G.POOL_MAX, 9, 9, 1, 1, 0, 0), "pool_2d: a 9x9 kernel at pad 0 does not fit the 9x7 input"),
                      ((2, 3, 3, 1, 1, 0, 0), r"pool_2d: kind 2 \(0 max, 1 average\)")]:
        with pytest.raises(L.Error, match=msg):
            G.pool_2d(m, x, *args)
    with pytest.raises(L.Error, match="pool_2d: C = 12 must be a multiple of 8"):
        G.pool_2d(m, g.input((12, 9, 7, 2), G.F16, "x12"), G.POOL_MAX, 3, 3, 1, 1, 1, 1)
    with pytest.raises(L.Error, match="pool_2d: a 3x3 kernel at pad 0 does not fit the 19x2 input"):  # (avg, 3, 1, 0, 40, 2, 19, 3): an empty output
        G.pool_2d(m, g.input((40, 19, 2, 3), G.F16, "thin"), G.POOL_AVG, 3, 3, 1, 1, 0, 0)
    for n in (12, 1032):
        with pytest.raises(L.Error, match=rf"soft_max: rows of {n} elements \(a multiple of 8, at most 1024\)"):
            G.soft_max(m, g.input((n, 3), G.F16, f"r{n}"))
    xf = g.input((16, 9, 7, 2), G.F32, "xf32")
    for name, fn in [("silu", lambda: G.silu(m, xf)), ("pool_2d", lambda: G.pool_2d(m, xf, G.POOL_MAX, 3, 3, 1, 1, 1, 1)), ("soft_max", lambda: G.soft_max(m, xf)),
                     ("sum_rows", lambda: G.sum_rows(m, xf)), ("sub", lambda: G.sub(m, x, xf))]:
        with pytest.raises(L.Error, match=f"{name}: operand [01] is f32"):
            fn()
    with pytest.raises(L.Error, match="sub: cannot broadcast"):
        G.sub(m, g.input((16, 1, 1, 1), G.F16, "small"), x)  # not commutative: the operands are not swapped


# ---- planned launch lists ----------------------------------------------------------------------------------------------------------------------

def test_a_silu_conv_is_one_launch(gguf):
    g = _plan(gguf, lambda g, m: [G.yolo_conv(m, _x(g, 16), "model.1", 3, 2)])
    assert _lines(g) == ["conv3x3s2[silu] M=60 N=32 K=144 <- model.1.conv.weight"]
    g = _plan(gguf, lambda g, m: [G.yolo_conv(m, g.input((3, 12, 10, 2), G.F32, "image"), "model.0", 3, 2)])
    assert _lines(g) == ["image_pad8 [3, 12, 10, 2]", "conv3x3s2[silu] M=60 N=16 K=72 <- model.0.conv.weight"]
    assert _lines(_plan(gguf, lambda g, m: [G.yolo_conv(m, _x(g, 16), "model.1", 3, 2)], False)) == ["conv3x3s2 M=60 N=32 K=144 <- model.1.conv.weight", "silu n=1920"]


def test_a_linear_and_its_silu_are_one_launch():
    def build(g, m):
        g.add_weight("fc.weight", np.zeros((24, 64), np.float32))
        return [G.silu(m, G.linear(G.ModelRef(g, "fc"), g.input((64, 10, 2), G.F16, "x")))]
    assert _lines(_plan(None, build)) == ["gemm[silu] M=20 N=24 K=64 <- fc.weight"]
    assert _lines(_plan(None, build, False)) == ["gemm M=20 N=24 K=64 <- fc.weight", "silu n=480"]


def test_elan1_is_four_convs(gguf):
    lines = _lines(_plan(gguf, lambda g, m: [G.yolo_elan1(m, _x(g, 32), "model.2", 32, 32, 32, 16)]))
    assert lines == ["conv1x1[silu][out ch 0..32 of 64] M=216 N=32 K=32 <- model.2.cv1.conv.weight",
                     "conv3x3[in ch 16..32 of 64][silu][out ch 32..48 of 64] M=216 N=16 K=144 <- model.2.cv2.conv.weight",
                     "conv3x3[in ch 32..48 of 64][silu][out ch 48..64 of 64] M=216 N=16 K=144 <- model.2.cv3.conv.weight",
                     "conv1x1[silu] M=216 N=32 K=64 <- model.2.cv4.conv.weight"]


def test_aconv_is_the_pool_and_the_conv(gguf):
    assert _lines(_plan(gguf, lambda g, m: [G.yolo_aconv(m, _x(g, 32), "model.3")])) == ["pool_avg2x2 B=2 12x9 -> 11x8 C=32 pad=0", "conv3x3s2[silu] M=48 N=64 K=288 <- model.3.cv1.conv.weight"]


def test_rep_ncsp_elan4_is_22_convs(gguf):
    g = _plan(gguf, lambda g, m: [G.yolo_rep_ncsp_elan4(m, _x(g, 64), "model.4", 64, 64, 64, 32, 3)])
    lines = _lines(g)
    assert len(lines) == 22 and all(l.startswith("conv") for l in lines), lines
    assert not [l for l in lines if l.split()[0] in ("silu", "add", "slice", "concat")]
    assert sum("[+conv1x1 folded][silu]" in l for l in lines) == 6 and sum("[silu][+res]" in l for l in lines) == 6
    assert lines[1] == "conv1x1[in ch 32..64 of 128][silu] M=216 N=16 K=32 <- model.4.cv2.0.cv1.conv.weight"
    assert lines[8] == "conv3x3[silu][+res][out ch 0..16 of 32] M=216 N=16 K=144 <- model.4.cv2.0.m.2.cv2.conv.weight"
    assert g.summary()["buffers"] < 22  # every concat is one buffer its producers write into


def test_sppelan_is_two_convs_and_three_pools(gguf):
    lines = _lines(_plan(gguf, lambda g, m: [G.yolo_sppelan(m, _x(g, 128, 3, 3), "model.9", 128, 128, 64)]))
    assert [l.split()[0].split("[")[0] for l in lines] == ["conv1x1", "pool_max5x5", "pool_max5x5", "pool_max5x5", "conv1x1"], lines
    assert lines[2] == "pool_max5x5[in ch 64..128 of 256][out ch 128..192 of 256] B=2 3x3 -> 3x3 C=64 pad=2"


def _dfl(g, m, n=16, nc=16):
    x = g.input((4 * n + nc, 37, 1, 2), G.F16, "x")
    proj = g.add_weight("proj", np.arange(n, dtype=np.float32), G.F32)
    return [G.yolo_dfl_forward(m, proj, G.cont(m, G.slice_(m, x, (0, 4 * n))), n)]


def test_the_dfl_chain_is_one_launch():
    g = _plan(None, _dfl)
    assert _lines(g) == ["softmax_expect rows=74 groups=4 n=16 [in ch 0..64 of 80]"]
    assert _lines(_plan(None, _dfl, False)) == ["slice [80, 37, 1, 2] -> [64, 37, 1, 2]", "soft_max rows=296 n=16", "mul n=4736 period=16 (constant)", "sum_rows rows=296 n=16"]

    def second_reader(g, m):  # the softmax has another reader: nothing is absorbed
        x = g.input((64, 37, 1, 2), G.F16, "x")
        soft = G.soft_max(m, G.reshape(m, x, 16, 4, 37, 2))
        return [G.sum_rows(m, G.mul(m, soft, g.add_weight("proj", np.arange(16, dtype=np.float32), G.F32))), soft]
    assert [l.split()[0] for l in _lines(_plan(None, second_reader))] == ["soft_max", "mul", "sum_rows"]


def test_per_node_every_node_is_its_own_launch(gguf):
    for build, ops in [(lambda g, m: [G.yolo_elan1(m, _x(g, 32), "model.2", 32, 32, 32, 16)], dict(silu=4, slice=2, concat=6, conv=2 + 2)),
                       (lambda g, m: [G.yolo_aconv(m, _x(g, 32), "model.3")], dict(pool=1, conv=1, silu=1)),
                       (lambda g, m: [G.yolo_sppelan(m, _x(g, 128, 3, 3), "model.9", 128, 128, 64)], dict(pool=3, conv=2, silu=2, concat=6)),
                       (lambda g, m: [G.yolo_rep_ncsp_elan4(m, _x(g, 64), "model.4", 64, 64, 64, 32, 3)], dict(silu=22, slice=2, conv=28))]:
        lines = _lines(_plan(gguf, build, False))
        assert not [l for l in lines if "[silu]" in l or "folded" in l or " ch " in l], lines
        count = lambda p: sum(l.startswith(p) for l in lines)
        got = dict(silu=count("silu "), slice=count("slice "), concat=count("concat "), pool=count("pool_"), conv=count("conv") + count("gemm(conv1x1)"))
        assert {k: got[k] for k in ops} == ops, (got, lines)


# ---- what must not fuse ----------------------------------------------------------------------------------------------------------------------------

def test_a_silu_whose_conv_has_a_second_reader_stays_a_launch(gguf):
    def build(g, m):
        c = G.conv_2d(G.ModelRef(g, "model.1.conv"), _x(g, 16), 2, 1)
        return [G.silu(m, c), G.scale(m, c, 2.0)]
    assert [l.split()[0] for l in _lines(_plan(gguf, build))] == ["conv3x3s2", "silu", "scale"]


def test_a_rep_conv_on_two_maps_or_with_a_second_reader_is_not_folded(gguf):
    p = "model.4.cv2.0.m.0.cv1"

    def two_maps(g, m):
        a = G.yolo_conv(m, _x(g, 16, name="a"), p + ".conv1.conv", 3, 1, False)
        b = G.yolo_conv(m, _x(g, 16, name="b"), p + ".conv2.conv", 1, 1, False)
        return [G.silu(m, G.add(m, a, b))]
    lines = _lines(_plan(gguf, two_maps))
    assert not [l for l in lines if "folded" in l] and sum(l.startswith(("conv", "gemm")) for l in lines) == 2, lines

    def second_reader(g, m):
        x = _x(g, 16)
        a = G.yolo_conv(m, x, p + ".conv1.conv", 3, 1, False)
        b = G.yolo_conv(m, x, p + ".conv2.conv", 1, 1, False)
        return [G.silu(m, G.add(m, a, b)), G.scale(m, b, 2.0)]
    lines = _lines(_plan(gguf, second_reader))
    assert not [l for l in lines if "folded" in l] and sum(l.startswith(("conv", "gemm")) for l in lines) == 2, lines

    def folded(g, m):
        return [G.yolo_rep_conv(m, _x(g, 16), p)]
    assert _lines(_plan(gguf, folded)) == [f"conv3x3[+conv1x1 folded][silu] M=216 N=16 K=144 <- {p}.conv1.conv.weight"]


def test_a_channel_slice_at_an_offset_of_four_is_copied(gguf):
    def build(c0):
        def b(g, m):
            g.add_weight("k.weight", np.zeros((8, 3, 3, 8), np.float32))
            return [G.silu(m, G.conv_2d(G.ModelRef(g, "k"), G.slice_(m, _x(g, 32), (c0, c0 + 8)), 1, 1))]
        return b
    assert _lines(_plan(None, build(4))) == ["slice [32, 12, 9, 2] -> [8, 12, 9, 2]", "conv3x3[silu] M=216 N=8 K=72 <- k.weight"]
    assert _lines(_plan(None, build(8))) == ["conv3x3[in ch 8..16 of 32][silu] M=216 N=8 K=72 <- k.weight"]


def _reshape_cases():
    """readers of a reshape that changes ne[0] (space-to-depth by reshape): the reshaped map is contiguous, its pixels are as wide as the reshape says"""
    def pool(g, m):
        return [G.pool_2d(m, G.reshape(m, _x(g, 16, 4, 4, 1), 8, 8, 4, 1), G.POOL_MAX, 3, 3, 1, 1, 1, 1)]

    def conv(g, m):
        g.add_weight("k.weight", np.zeros((8, 3, 3, 8), np.float32))
        return [G.silu(m, G.conv_2d(G.ModelRef(g, "k"), G.reshape(m, _x(g, 16, 4, 4, 1), 8, 8, 4, 1), 1, 1))]

    def sliced(g, m):  # channels 8..16 of the reshaped map
        g.add_weight("k.weight", np.zeros((8, 3, 3, 8), np.float32))
        return [G.silu(m, G.conv_2d(G.ModelRef(g, "k"), G.slice_(m, G.reshape(m, _x(g, 32, 4, 4, 1), 16, 8, 4, 1), (8, 16)), 1, 1))]

    def reshaped_slice(g, m):  # a reshape of a channel slice is not read in place: the slice is copied
        return [G.pool_2d(m, G.reshape(m, G.slice_(m, _x(g, 32, 4, 4, 1), (16, 32)), 8, 8, 4, 1), G.POOL_MAX, 3, 3, 1, 1, 1, 1)]
    return pool, conv, sliced, reshaped_slice


def test_readers_of_a_reshape_take_the_reshaped_width():
    pool, conv, sliced, reshaped_slice = _reshape_cases()
    assert _lines(_plan(None, pool)) == _lines(_plan(None, pool, False)) == ["pool_max3x3 B=1 8x4 -> 8x4 C=8 pad=1"]
    assert _lines(_plan(None, conv)) == ["conv3x3[silu] M=32 N=8 K=72 <- k.weight"]
    assert _lines(_plan(None, sliced)) == ["conv3x3[in ch 8..16 of 16][silu] M=32 N=8 K=72 <- k.weight"]
    assert _lines(_plan(None, reshaped_slice)) == ["slice [32, 4, 4, 1] -> [16, 4, 4, 1]", "pool_max3x3 B=1 8x4 -> 8x4 C=8 pad=1"]


def test_a_silu_conv_on_an_f32_activation_is_refused_not_matched():
    g = G.Graph(None)
    g.add_weight("k.weight", np.zeros((8, 3, 3, 16), np.float32))
    with pytest.raises(L.Error, match="conv_2d: operand 0 is f32"):
        G.conv_2d(G.ModelRef(g, "k"), g.input((16, 4, 4, 1), G.F32, "xf"), 2, 1)
    # the one f32 activation a conv may read besides the 3-channel image, an image of up to 16 channels under a 3x3 / s1 / p1 kernel, stays with the
    # LDS-ring conv that reads it as value | residue planes; its silu is a launch
    def image8(g, m):
        g.add_weight("k8.weight", np.zeros((32, 3, 3, 8), np.float32))
        return [G.silu(m, G.conv_2d(G.ModelRef(g, "k8"), g.input((8, 20, 20, 1), G.F32, "img8"), 1, 1))]
    lines = _lines(_plan(None, image8))
    assert lines[0].startswith("image_planes") and lines[1].startswith("dconv3x3(planes)[f32 image]") and lines[-1] == "silu n=12800" and not [l for l in lines if "[silu]" in l], lines


def test_a_concat_without_a_placeable_source_plans_as_before():
    def build(g, m):
        return [G.concat(m, [G.relu(m, _x(g, 16, name="a")), G.scale(m, _x(g, 8, name="b"), 2.0)], 0)]
    assert _lines(_plan(None, build)) == ["relu n=3456", "scale n=1728", "concat part 0 [16, 12, 9, 2] -> [24, 12, 9, 2]", "concat part 1 [8, 12, 9, 2] -> [24, 12, 9, 2]"]


def test_a_nearest_resize_alone_plans_as_before():
    assert _lines(_plan(None, lambda g, m: [G.upscale(m, _x(g, 16), 2, G.SCALE_MODE_NEAREST)])) == ["nearest 12x9 -> 24x18 C=16"]


def test_a_pool_writes_into_a_concat_and_an_output_is_not_placed():
    def build(g, m):
        x = _x(g, 16)
        r = G.relu(m, x)
        p = G.pool_2d(m, x, G.POOL_MAX, 3, 3, 1, 1, 1, 1)
        return [G.concat(m, [r, p], 0)]
    assert _lines(_plan(None, build)) == ["relu n=3456", "pool_max3x3[out ch 16..32 of 32] B=2 12x9 -> 12x9 C=16 pad=1", "concat part 0 [16, 12, 9, 2] -> [32, 12, 9, 2]"]

    def build_out(g, m):
        x = _x(g, 16)
        r = G.relu(m, x)
        p = G.pool_2d(m, x, G.POOL_MAX, 3, 3, 1, 1, 1, 1)
        return [G.concat(m, [r, p], 0), p]
    assert [l.split()[0] for l in _lines(_plan(None, build_out))] == ["relu", "pool_max3x3", "concat", "concat"]


# ---- the whole network --------------------------------------------------------------------------------------------------------------------------

def _is_conv(l):
    return l.startswith("conv") or l.startswith("gemm(conv1x1)")


def test_the_conv_network_at_96_has_at_most_185_convs_and_no_silu_or_slice_launch(gguf):
    def build(g, m):
        f = G.yolov9t_backbone(m, g.input((3, 96, 96, 2), G.F32, "image"))
        assert [f[i].ne[1] for i in (0, 1, 3, 5, 7)] == [48, 24, 12, 6, 3]
        return G.yolo_detect_forward(m, [f[15], f[18], f[21]], [64, 96, 128], 80, training=True)[2]
    lines = _lines(_plan(gguf, build))
    convs = sum(_is_conv(l) for l in lines)
    assert convs == 185, convs  # what csrc/yolov9t.cpp launches: the network's 227 convs with the 42 1x1 branches of its RepConvs folded
    assert not [l for l in lines if l.split()[0] in ("silu", "slice", "add")], lines
    others = [l.split()[0].split("[")[0] for l in lines if not _is_conv(l)]
    assert sorted(others) == sorted(["image_pad8"] + ["pool_avg2x2"] * 5 + ["pool_max5x5"] * 3 + ["nearest"] * 2), others  # no channel concat is copied
    assert [l for l in lines if l.startswith("nearest")] == ["nearest[in ch 64..192 of 192][out ch 0..128 of 224] 3x3 -> 6x6 C=128",
                                                             "nearest[in ch 48..144 of 144][out ch 0..96 of 160] 6x6 -> 12x12 C=96"]


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "per_node"])
def test_the_whole_network_at_96(gguf, fused):
    def build(g, m):
        boxes, scores, raw, f = G.yolov9t_forward(m, g.input((3, 96, 96, 2), G.F32, "image"))
        assert boxes.ne == (4, 189, 1, 2) and scores.ne == (80, 189, 1, 2) and [r.ne for r in raw] == [(144, 12, 12, 2), (144, 6, 6, 2), (144, 3, 3, 2)]
        return [boxes, scores, *raw, *(f[i] for i in (2, 4, 9, 15, 21))]
    lines = _lines(_plan(gguf, build, fused))
    convs = sum(_is_conv(l) for l in lines)
    if fused:
        assert convs <= 185, convs
        assert not [l for l in lines if l.startswith("silu ")], lines
        assert sum(l.startswith("softmax_expect") for l in lines) == 1 and not [l for l in lines if l.startswith(("soft_max", "sum_rows"))]
        # the decode's three: the class logits (read by sigmoid) and dist2bbox's lt / rb (two channels each)
        assert [l for l in lines if l.startswith("slice ")] == ["slice [144, 189, 1, 2] -> [80, 189, 1, 2]"] + ["slice [4, 189, 1, 2] -> [2, 189, 1, 2]"] * 2
    else:
        assert convs == 227 and sum(l.startswith("silu ") for l in lines) == 179 and sum(l.startswith("soft_max") for l in lines) == 1


def test_cpp_face_builds_the_same_blocks(gguf):
    """tests/cpp/yolov9t_graph_check.cpp: SPPELAN and RepNCSPELAN4 through include/visp/nn.h, planned on the host; the launch lists equal the Python face's."""
    exe = ROOT / "vision.cpp_amd" / "lib" / "yolov9t_graph_check"
    assert exe.exists(), "built by __graft_entry__.build()"
    for fused in (True, False):
        for kind, prefix, shape, build in [("sppelan", "model.9", (128, 64, 64, 3, 3, 2), lambda g, m: [G.yolo_sppelan(m, _x(g, 128, 3, 3), "model.9", 128, 128, 64)]),
                                           ("elan4", "model.4", (64, 64, 32, 12, 9, 2), lambda g, m: [G.yolo_rep_ncsp_elan4(m, _x(g, 64), "model.4", 64, 64, 64, 32, 3)])]:
            r = subprocess.run([str(exe), str(gguf), kind, prefix, *map(str, shape), str(int(fused))], capture_output=True, text=True, timeout=120)
            assert r.returncode == 0, (r.stdout, r.stderr)
            assert r.stdout == _plan(gguf, build, fused).describe(), (kind, fused)


"""-m gpu: each generic op of the graph executor through `Graph(device)` at edge shapes (odd channel counts that take the scalar kernels, strided
and negative slices, concat on every dimension with a constant part, broadcasts of every legal period), against tests/graph_ref.py; then the
fusion near-misses of tests/graph_cases.py, whose lowering tests/test_graph_cpu.py pins, against torch or the per-node lowering."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import graph_cases as GC
import graph_ref as R
from visioncpp_amd import graph as G
from visioncpp_amd import vision

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def device():
    return vision.Device.init(vision.Backend.gpu)


def run(g, feeds, outs):
    g.allocate()
    for k, v in feeds.items():
        g.set(k, v)
    g.compute()
    return [g.get(o) for o in outs]


def rand16(rng, *shape, s=2.0):
    return R.f16(rng.standard_normal(shape) * s)


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))


# ---- element-wise ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("C", [3, 5, 8])
@pytest.mark.parametrize("op", ["add", "mul"])
def test_binary_with_constants_of_every_period_and_an_activation(device, C, op):
    """a (op) b for b a constant of each legal broadcast shape (period 1, C, C W, C W H, everything) and b another activation, same shape or
    broadcast: within 1 f16 ulp of the float64 result."""
    rng = np.random.default_rng(C)
    W, H, B = 7, 3, 2
    x = rand16(rng, B, H, W, C)
    shapes = [(1,), (C,), (W, C), (H, W, C), (B, H, W, C)]
    g = G.Graph(device)
    m = G.ModelRef(g)
    xi = g.input((C, W, H, B), G.F16)
    zi = g.input((C, W, 1, 1), G.F16)
    z = rand16(rng, 1, 1, W, C)
    fn = G.add if op == "add" else G.mul
    consts, outs = [], []
    for i, sh in enumerate(shapes):
        b = R.f16(rng.standard_normal(sh))
        consts.append(b)
        outs.append(g.output(fn(m, xi, g.add_weight(f"b{i}", b, G.F32)), f"y{i}"))
    outs.append(g.output(fn(m, xi, xi), "self"))
    outs.append(g.output(fn(m, xi, zi), "bcast"))
    got = run(g, {xi: x, zi: z}, outs)
    for i, b in enumerate(consts):
        R.assert_f16_ulp(got[i], getattr(R, op)(x, b), 1.0, f"{op} constant {b.shape}")
    R.assert_f16_ulp(got[-2], getattr(R, op)(x, x), 1.0, f"{op} self")
    R.assert_f16_ulp(got[-1], getattr(R, op)(x, z), 1.0, f"{op} broadcast activation")


@pytest.mark.parametrize("C", [3, 5, 16])
def test_unary_nodes(device, C):
    """gelu / relu / scale / leaky_relu (slopes 1.5 and -0.5: ggml's x > 0 ? x : s x) on maps whose element count is not a multiple of 8."""
    rng = np.random.default_rng(10 + C)
    W, H, B = 5, 3, 1
    x = rand16(rng, B, H, W, C, s=3.0)
    g = G.Graph(device)
    m = G.ModelRef(g)
    xi = g.input((C, W, H, B), G.F16)
    ys = [g.output(G.gelu(m, xi), "gelu"), g.output(G.relu(m, xi), "relu"), g.output(G.scale(m, xi, -0.3), "scale"),
          g.output(G.leaky_relu(m, xi, 1.5), "l15"), g.output(G.leaky_relu(m, xi, -0.5), "lm05")]
    ge, re_, sc, l1, l2 = run(g, {xi: x}, ys)
    R.assert_f16_ulp(ge, R.gelu(x), R.GELU_F16_ULPS, "gelu")
    np.testing.assert_array_equal(re_, R.relu(x))
    R.assert_f16_ulp(sc, R.scale(x, -0.3), 1.0, "scale")
    R.assert_f16_ulp(l1, R.leaky_relu(x, 1.5), 1.0, "leaky 1.5")
    R.assert_f16_ulp(l2, R.leaky_relu(x, -0.5), 1.0, "leaky -0.5")
    np.testing.assert_array_equal(l1[x > 0], x[x > 0])


@pytest.mark.parametrize("C", [8, 520, 1024])
def test_layer_norm_node(device, C):
    """f32 statistics (two passes) over C f16 values, then f16: within 1 f16 ulp plus 4 C u (|w x^| + |b|)."""
    rng = np.random.default_rng(C)
    rows = 37
    x = rand16(rng, rows, C)
    w = (1 + 0.2 * rng.standard_normal(C)).astype(np.float32)
    b = (0.1 * rng.standard_normal(C)).astype(np.float32)
    g = G.Graph(device)
    g.add_weight("n.weight", w, G.F32); g.add_weight("n.bias", b, G.F32)
    xi = g.input((C, rows), G.F16)
    (got,) = run(g, {xi: x}, [g.output(G.layer_norm(G.ModelRef(g)["n"], xi, 1e-6), "y")])
    want = R.layer_norm(x, w, b, 1e-6)
    slack = 4 * C * 2.0 ** -24 * (np.abs(want - b) + np.abs(b))
    assert (np.abs(got - R.f16(want)) <= R.f16_ulp(want) + slack).all()


# ---- data movement (exact) ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("C", [3, 5, 16])
def test_slices(device, C):
    """Steps, negative begins and odd offsets (a misaligned source for the strided copy); exact."""
    rng = np.random.default_rng(20 + C)
    W, H, B = 11, 6, 3
    x = rand16(rng, B, H, W, C)
    sels = [((1, C, 2), (-5, W), G.SLICE_ALL, G.SLICE_ALL), (G.SLICE_ALL, (1, W, 3), (-4, -1), (1, 3)), ((C - 1, C), (0, W, 2), (1, H, 2), (-1, B)),
            (G.SLICE_ALL, 3, G.SLICE_ALL, G.SLICE_ALL)]
    g = G.Graph(device)
    m = G.ModelRef(g)
    xi = g.input((C, W, H, B), G.F16)
    outs = [g.output(G.slice_(m, xi, *s), f"s{i}") for i, s in enumerate(sels)]
    got = run(g, {xi: x}, outs)
    for gv, s in zip(got, sels):
        want = R.slice_(x, *[None if v == G.SLICE_ALL else v for v in s])
        np.testing.assert_array_equal(gv, want)


@pytest.mark.parametrize("dim", [0, 1, 2, 3])
@pytest.mark.parametrize("C", [3, 8])
def test_concat_with_a_constant_part(device, dim, C):
    """concat along each dimension of an activation and a constant (the constant's f16 image), in both orders; exact."""
    rng = np.random.default_rng(dim + C)
    ne = [C, 5, 4, 2]
    x = rand16(rng, *ne[::-1])
    cne = list(ne)
    cne[dim] = 3
    c = R.f16(rng.standard_normal(cne[::-1]))
    g = G.Graph(device)
    m = G.ModelRef(g)
    xi = g.input(tuple(ne), G.F16)
    ct = g.add_weight("c", c, G.F16)
    a = g.output(G.concat(m, [xi, ct], dim), "a")
    b = g.output(G.concat(m, [ct, xi, xi], dim), "b")
    ga, gb = run(g, {xi: x}, [a, b])
    np.testing.assert_array_equal(ga, R.concat(x, c, dim))
    np.testing.assert_array_equal(gb, R.concat(R.concat(c, x, dim), x, dim))


@pytest.mark.parametrize("C", [3, 8])
def test_repeat_with_broadcast(device, C):
    rng = np.random.default_rng(30 + C)
    x = rand16(rng, 1, 4, 1, C)
    g = G.Graph(device)
    m = G.ModelRef(g)
    xi = g.input((C, 1, 4, 1), G.F16)
    (got,) = run(g, {xi: x}, [g.output(G.repeat(m, xi, C, 6, 4, 3), "y")])
    np.testing.assert_array_equal(got, R.repeat(x, C, 6, 4, 3))


@pytest.mark.parametrize("size", [(5, 9, 9, 5), (7, 3, 3, 7), (19, 37, 37, 19), (6, 13, 8, 4)])
def test_nearest_node(device, size):
    """interpolate NEAREST at non-integer ratios, different in W and H; exact against ggml's index."""
    W, OW, H, OH = size
    rng = np.random.default_rng(W * OW)
    x = rand16(rng, 2, H, W, 8)
    g = G.Graph(device)
    xi = g.input((8, W, H, 2), G.F16)
    (got,) = run(g, {xi: x}, [g.output(G.interpolate(G.ModelRef(g), xi, (OW, OH), G.SCALE_MODE_NEAREST), "y")])
    np.testing.assert_array_equal(got, R.interpolate_nearest(x, OW, OH))


@pytest.mark.parametrize("kind", ["constant", "one_pixel", "random"])
def test_image_ops(device, kind):
    """image_u8_to_f32 on a constant image, a one-pixel image and a random one; image_normalize on a constant map (span below 1e-5: the map minus
    its minimum), a one-pixel map and a random one. Both exact against the f32 steps the kernels take. (The two do not chain: image_normalize reads
    a one-channel map.)"""
    rng = np.random.default_rng(len(kind))
    W, H, B = {"constant": (9, 7, 2), "one_pixel": (1, 1, 2), "random": (13, 5, 3)}[kind]
    img = np.full((B, H, W, 3), 77, np.uint8) if kind == "constant" else rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)
    d = np.full((B, H, W, 1), 0.3, np.float32) if kind == "constant" else rng.standard_normal((B, H, W, 1)).astype(np.float32)
    mean, istd = [0.485, 0.456, 0.406], [1 / 0.229, 1 / 0.224, 1 / 0.225]
    g = G.Graph(device)
    u8 = g.input((3, W, H, B), G.U8, "u8")
    dm = g.input((1, W, H, B), G.F32, "d")
    a = g.output(g.op(G.OP_IMAGE_U8_TO_F32, [u8], fparams=mean + istd), "a")
    n = g.output(g.op(G.OP_IMAGE_NORMALIZE, [dm]), "n")
    ga, gn = run(g, {u8: img, dm: d}, [a, n])
    np.testing.assert_array_equal(ga.view(np.uint32), R.image_u8_to_f32(img, mean, istd).view(np.uint32))
    np.testing.assert_array_equal(gn, R.image_normalize(d))


# ---- fusion near-misses ------------------------------------------------------------------------------------------------------

def conv_t(v, w, b):
    return F.conv2d(v, t(w).permute(0, 3, 1, 2), t(b), padding=1)


@pytest.mark.parametrize("cout", [64, 32])
def test_conv_relu_add_numbers(device, cout):
    rng = np.random.default_rng(cout)
    g = G.Graph(device)
    c = GC.conv_relu_add(g, rng, cout)
    x, o = R.f16(rng.standard_normal((2, 18, 20, 64))), R.f16(rng.standard_normal((2, 18, 20, cout)))
    (got,) = run(g, {c["x"]: x, c["other"]: o}, [c["y"]])
    r = torch.relu(conv_t(t(x).permute(0, 3, 1, 2), c["w"], c["b"])).permute(0, 2, 3, 1).numpy()
    want = R.f16(r).astype(np.float64) + o
    assert np.abs(got - want).max() <= 4e-3 * np.abs(want).max()  # f32 products over K = 576 f16 terms, two f16 roundings


def test_residual_unit_on_planes_numbers(device):
    rng = np.random.default_rng(6)
    g = G.Graph(device)
    c = GC.residual_unit_on_planes(g, rng)
    img = rng.random((2, 18, 20, 3)).astype(np.float32)
    (got,) = run(g, {c["image"]: img}, [c["y"]])
    (w0, b0), (w1, b1), (w2, b2) = c["w"]
    x0 = t(R.f16(conv_t(t(img).permute(0, 3, 1, 2), w0, b0).numpy()))
    o = t(R.f16(torch.relu(conv_t(torch.relu(x0), w1, b1)).numpy()))
    want = (x0 + conv_t(o, w2, b2)).permute(0, 2, 3, 1).numpy()
    assert np.abs(got - want).max() <= 4e-3 * np.abs(want).max()


@pytest.mark.parametrize("planar", [False, True])
def test_relu_into_output_conv_numbers(device, planar):
    rng = np.random.default_rng(7)
    g = G.Graph(device)
    c = GC.relu_into_output_conv(g, rng, planar)
    if planar:
        src = rng.random((2, 18, 20, 3)).astype(np.float32)
        got_y, got_x0 = run(g, {c["src"]: src}, [c["y"], c["x0"]])
        x = t(R.f16(conv_t(t(src).permute(0, 3, 1, 2), *c["w0"]).numpy()))
        np.testing.assert_allclose(got_x0, x.permute(0, 2, 3, 1).numpy(), atol=4e-3 * float(x.abs().max()))
    else:
        src = R.f16(rng.standard_normal((2, 18, 20, 64)))
        (got_y,) = run(g, {c["src"]: src}, [c["y"]])
        x = t(src).permute(0, 3, 1, 2)
    want = conv_t(torch.relu(x), *c["w1"]).permute(0, 2, 3, 1).numpy()
    assert np.abs(got_y - want).max() <= 4e-3 * np.abs(want).max()


@pytest.mark.parametrize("slope", [0.1, 1.5, -0.5])
def test_conv_leaky_numbers(device, slope):
    rng = np.random.default_rng(8)
    g = G.Graph(device)
    c = GC.conv_leaky(g, rng, slope)
    x = R.f16(rng.standard_normal((2, 18, 20, 64)))
    (got,) = run(g, {c["x"]: x}, [c["y"]])
    r = R.f16(conv_t(t(x).permute(0, 3, 1, 2), c["w"], c["b"]).permute(0, 2, 3, 1).numpy())
    want = R.leaky_relu(r, slope)
    assert np.abs(got - want).max() <= 4e-3 * np.abs(want).max()


@pytest.mark.parametrize("cin", [16, 48])
def test_conv_narrow_input_numbers(device, cin):
    """Cin = 16 (below the LDS-ring conv's pixel stride: the GEMM family's conv) and Cin = 48 (the LDS-ring conv on weights padded to 64, the
    last pixel's missing channels zero-filled by its loader) against the float64 conv: the f32 sum of K = 9 cin f16 products in any order is within
    (K + 8) 2^-24 of the sum of magnitudes, then one f16 rounding."""
    rng = np.random.default_rng(cin)
    g = G.Graph(device)
    c = GC.conv_narrow_input(g, rng, cin)
    x = R.f16(rng.standard_normal((2, 18, 20, cin)))
    (got,) = run(g, {c["x"]: x}, [c["y"]])
    want = R.conv3x3(x, c["w"], c["b"])
    mag = R.conv3x3(np.abs(x), np.abs(c["w"]), np.abs(c["b"]))
    assert got.shape == want.shape and np.isfinite(got).all()
    assert (np.abs(got - want) <= (9 * cin + 8) * 2.0 ** -24 * mag + np.maximum(2.0 ** -11 * np.abs(want), 2.0 ** -25)).all()


@pytest.mark.parametrize("scales", [(0.125, 0.125), (0.125, 0.5)])
def test_encoder_chain_matches_the_per_node_lowering(device, scales):
    """The two-layer chain lowered with the model kernels (dino_block when the scales agree) and node by node agree to f16 rounding of the
    intermediates; a chain with a different scale in layer 1 gives the same numbers both ways because it is not fused with layer 0's scale."""
    rng = np.random.default_rng(9)
    img = rng.standard_normal((2, 28, 28, 3)).astype(np.float32)
    res = {}
    for fused in (True, False):
        g = G.Graph(device)
        g.set_fused_models(fused)
        c = GC.encoder_chain(g, np.random.default_rng(11), scales)
        (res[fused],) = run(g, {c["image"]: img}, [c["y"]])
        assert ("dino_block[" in g.describe()) == (fused and scales[0] == scales[1])
    d = np.abs(res[True] - res[False])
    assert d.max() <= 2e-2 * np.abs(res[False]).max() and d.mean() < 2e-3, (float(d.max()), float(d.mean()))
    # the scale matters: the same chain with layer 1 at layer 0's scale is far from this one
    if scales[0] != scales[1]:
        g = G.Graph(device)
        c = GC.encoder_chain(g, np.random.default_rng(11), (scales[0], scales[0]))
        (other,) = run(g, {c["image"]: img}, [c["y"]])
        assert np.abs(other - res[False]).mean() > 10 * d.mean() + 1e-3


def test_nearest_agrees_with_torch_where_the_indices_do(device):
    """torch's nearest uses floor(i * in / out); where that picks the same source as ggml's floor(i / (out / in)), the values agree."""
    rng = np.random.default_rng(12)
    W, H, OW, OH = 7, 5, 16, 9
    x = rand16(rng, 1, H, W, 8)
    g = G.Graph(device)
    xi = g.input((8, W, H, 1), G.F16)
    (got,) = run(g, {xi: x}, [g.output(G.interpolate(G.ModelRef(g), xi, (OW, OH), G.SCALE_MODE_NEAREST), "y")])
    tv = F.interpolate(t(x).permute(0, 3, 1, 2), size=(OH, OW), mode="nearest").permute(0, 2, 3, 1).numpy()
    ty, tx = np.floor(np.arange(OH) * (H / OH)).astype(int), np.floor(np.arange(OW) * (W / OW)).astype(int)
    agree = (ty == R.nearest_index(OH, H))[:, None] & (tx == R.nearest_index(OW, W))[None, :]
    assert agree.any()
    np.testing.assert_array_equal(got[:, agree], tv[:, agree])
    assert math.isfinite(float(got.sum()))

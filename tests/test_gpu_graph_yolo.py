"""-m gpu: the graph layer's pooling, SiLU, softmax, softmax-expectation and row-sum kernels (csrc/kernels_pool.hip, kernels_graph.hip), each directly and
through its node, and YOLOv9t built through vision.cpp_amd/graph.py::yolov9t_forward -- against float64 numpy on f16-rounded operands (tests/pool_ref.py)
and against tests/yolov9t_ref.py's restatement of src/visp/arch/yolov9t.cpp on f16-rounded weights, block by block and as a whole, fused and per node.

Bounds. Max pooling is bit-equal to float64: the maximum of f16 values is one of them. Average, SiLU, softmax, the softmax expectation and the row sum
are within 4 x the floor, the floor being the float64 result rounded to f16 against itself (the rule of DESIGN.md section 14): their f32 arithmetic
(sums of at most 1024 terms, v_exp / v_rcp at an ulp of f32) is far below one f16 rounding. Blocks and features: 2e-2 of the largest value; raw maps
5e-2 absolute; scores and boxes SCORE_TOL / BOX_TOL -- the bounds of tests/test_gpu_yolov9t.py for the hand schedule. At S = 96 a box coordinate is
below 128 px, where f16 values are 0.0625 px apart.

Measured on MI355X (DESIGN.md section 17 has all of it): every max case bit-equal; average 2.38e-4 and 3.86e-4, SiLU 1.77e-4 over |x| < 100, softmax 2.40e-4 /
2.24e-4 / 1.18e-4 / exact, softmax expectation 2.60e-4, row sums 2.13e-4 -- each equal to its floor; the DFL chain 2.60e-4 as one launch, 5.93e-4 per node.
Blocks fused / per node: elan1 4.48e-4 / 6.85e-4, rep_ncsp_elan4 6.43e-4 / 1.30e-3, sppelan 3.68e-4 / 6.30e-4, aconv 4.28e-4 / 5.08e-4. Network at S = 96: features
5.6e-4 .. 7.1e-4 fused, 7.5e-4 .. 1.02e-3 per node; raw maps at most 3.35e-3 / 3.96e-3; scores 4.34e-4 / 6.02e-4; boxes 0.176 / 0.265 px; 5.52e-4 and 0.219 px from
the hand schedule."""
import numpy as np
import pytest

import graph_ref
import pool_ref as R
import yolov9t_ref as Y
from visioncpp_amd import _lib as L
from visioncpp_amd import graph as G
from visioncpp_amd import synth, vision

pytestmark = pytest.mark.gpu

from gpu_util import api, dev, empty, release, sync  # noqa: E402

SCORE_TOL = 5e-3  # scores max abs (tests/test_gpu_yolov9t.py)
BOX_TOL = 1.0     # boxes max abs, input pixels


@pytest.fixture(scope="module")
def device():
    assert api().vx_device_count() > 0, "no HIP device visible: the product path has no CPU fallback"
    return vision.Device.init(vision.Backend.gpu)


@pytest.fixture(autouse=True)
def _release_buffers():
    yield
    release()


def _h(a):
    return np.asarray(a, np.float64).astype(np.float16)


# ---- vx_pool2d_f16 -----------------------------------------------------------------------------------------------------------------------------------

SLICE_CASE = 1  # read from channels 8..32 of a 40-channel map, written into channels 16..40 of a 48-channel buffer filled with 7.0
_pool_cache = {}


def _pool_case(i):
    """the input as f16 values (for SLICE_CASE the whole 40-channel map) and the float64 result, computed once and shared"""
    if i not in _pool_cache:
        kind, k, s, pad, C, H, W, B = R.POOL_CASES[i]
        x = R.f16(np.random.default_rng(300 + i).standard_normal((B, H, W, 40 if i == SLICE_CASE else C)))
        want = R.pool2d(x[..., 8:32] if i == SLICE_CASE else x, kind, k, s, pad)
        for a in (x, want):
            a.setflags(write=False)
        _pool_cache[i] = (x, want, R.f16_floor(want))
    return _pool_cache[i]


def _check_pool(i, got, want, floor, what):
    kind = R.POOL_CASES[i][0]
    assert got.shape == want.shape and np.isfinite(got.astype(np.float32)).all()
    if kind == R.MAX:
        np.testing.assert_array_equal(got.astype(np.float64), want)  # bit-equal
        print(f"pool {what} {R.POOL_CASES[i]}: bit-equal")
    else:
        err = R.rel_err(got, want)
        print(f"pool {what} {R.POOL_CASES[i]}: rel err {err:.3g} floor {floor:.3g} bound {4 * floor:.3g}")
        assert err <= 4 * floor, (R.POOL_CASES[i], err, floor)


@pytest.mark.parametrize("i", range(len(R.POOL_CASES)))
def test_pool_launcher_against_float64(i):
    kind, k, s, pad, C, H, W, B = R.POOL_CASES[i]
    x, want, floor = _pool_case(i)
    OH, OW = want.shape[1:3]
    xd = dev(_h(x))
    if i == SLICE_CASE:
        out = dev(np.full((B, OH, OW, 48), 7.0, np.float16))
        L.vx_check(api().vx_pool2d_f16(xd.ptr + 8 * 2, 40, out.ptr + 16 * 2, 48, B, H, W, C, kind, k, s, pad, None))
        sync()
        full = out.to_numpy(np.float16, (B, OH, OW, 48))
        assert (full[..., :16] == 7.0).all() and (full[..., 40:] == 7.0).all(), "the buffer outside the written slice was touched"
        got = full[..., 16:40]
    else:
        out = empty(want.size * 2, zero=False)
        L.vx_check(api().vx_pool2d_f16(xd.ptr, C, out.ptr, C, B, H, W, C, kind, k, s, pad, None))
        sync()
        got = out.to_numpy(np.float16, want.shape)
    _check_pool(i, got, want, floor, "launcher")


def test_pool_launcher_refuses_what_it_was_not_built_for():
    x = dev(np.zeros((1, 4, 4, 8), np.float16))
    y = empty(4 * 4 * 8 * 2)
    for args, msg in [((8, 8, 1, 4, 4, 12, 0, 3, 1, 1), b"multiple of 8"), ((8, 8, 1, 4, 4, 8, 0, 14, 1, 7), b"kernel 14"), ((8, 8, 1, 4, 4, 8, 0, 3, 3, 1), b"stride 3"),
                      ((8, 8, 1, 4, 4, 8, 0, 3, 1, 2), b"pad 2"), ((8, 8, 1, 4, 4, 8, 1, 3, 1, 1), b"average pooling with padding"), ((8, 8, 1, 4, 4, 8, 0, 5, 1, 0), b"does not fit"),
                      ((4, 8, 1, 4, 4, 8, 0, 3, 1, 1), b"pixel strides"), ((8, 8, 1, 4, 4, 8, 2, 3, 1, 1), b"kind 2")]:
        x_pix, y_pix, *rest = args
        assert api().vx_pool2d_f16(x.ptr, x_pix, y.ptr, y_pix, *rest, None) == 0 and msg in api().vx_last_error(), msg


@pytest.mark.parametrize("i", range(len(R.POOL_CASES)))
def test_pool_node_against_float64(device, i):
    kind, k, s, pad, C, H, W, B = R.POOL_CASES[i]
    x, want, floor = _pool_case(i)
    g = G.Graph(device)
    m = G.ModelRef(g)
    xi = g.input((x.shape[3], W, H, B), G.F16, "x")
    if i == SLICE_CASE:  # the slice is read where it lies and the pool writes into its part of the concat; the other part is a launch of its own
        OH, OW = want.shape[1:3]
        side = g.input((16, OW, OH, B), G.F16, "side")
        head = G.scale(m, side, 2.0)
        y = g.output(G.concat(m, [head, G.pool_2d(m, G.slice_(m, xi, (8, 32)), kind, k, k, s, s, pad, pad)], 0), "y")
        g.allocate()
        lines = g.describe().strip().splitlines()[:-1]
        assert lines == ["scale n=1232", "pool_max5x5[in ch 8..32 of 40][out ch 16..40 of 40] B=1 11x7 -> 11x7 C=24 pad=2", "concat part 0 [16, 11, 7, 1] -> [40, 11, 7, 1]"], lines
        sv = R.f16(np.random.default_rng(9).standard_normal((B, OH, OW, 16)))
        g.set(side, sv)
        g.set(xi, x)
        g.compute()
        got = g.get(y)
        np.testing.assert_array_equal(got[..., :16], 2.0 * sv)
        _check_pool(i, _h(got[..., 16:]), want, floor, "node")
        return
    y = g.output(G.pool_2d(m, xi, kind, k, k, s, s, pad, pad), "y")
    g.allocate()
    lines = g.describe().strip().splitlines()[:-1]
    assert len(lines) == 1 and lines[0].startswith(f"pool_{'max' if kind == R.MAX else 'avg'}{k}x{k}{'s2' if s == 2 else ''} "), lines
    g.set(xi, x)
    g.compute()
    _check_pool(i, _h(g.get(y)), want, floor, "node")


# ---- vx_nearest_pix_f16 ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B,H,W,OH,OW", [(2, 3, 5, 6, 10), (1, 4, 3, 7, 5)])
def test_nearest_with_pixel_strides_is_exact(device, B, H, W, OH, OW):
    """channels 8..32 of a 40-channel map into channels 16..40 of a 48-channel buffer filled with 7.0, at x2 and at a non-integer ratio; then the node:
    an upsample of a channel slice written into its part of a concat"""
    x = R.f16(np.random.default_rng(H * W).standard_normal((B, H, W, 40)))
    want = graph_ref.interpolate_nearest(x[..., 8:32], OW, OH)
    out = dev(np.full((B, OH, OW, 48), 7.0, np.float16))
    L.vx_check(api().vx_nearest_pix_f16(dev(_h(x)).ptr + 8 * 2, 40, out.ptr + 16 * 2, 48, B, H, W, 24, OH, OW, None))
    sync()
    full = out.to_numpy(np.float16, (B, OH, OW, 48))
    assert (full[..., :16] == 7.0).all() and (full[..., 40:] == 7.0).all(), "the buffer outside the written slice was touched"
    np.testing.assert_array_equal(full[..., 16:40].astype(np.float64), want)
    assert api().vx_nearest_pix_f16(out.ptr, 20, out.ptr, 48, B, H, W, 24, OH, OW, None) == 0 and b"pixel strides" in api().vx_last_error()
    g = G.Graph(device)
    m = G.ModelRef(g)
    xi, side = g.input((40, W, H, B), G.F16, "x"), g.input((16, OW, OH, B), G.F16, "side")
    head = G.scale(m, side, 2.0)
    y = g.output(G.concat(m, [head, G.interpolate(m, G.slice_(m, xi, (8, 32)), (OW, OH), G.SCALE_MODE_NEAREST)], 0), "y")
    g.allocate()
    lines = g.describe().strip().splitlines()[:-1]
    assert [l.split()[0] for l in lines] == ["scale", "nearest[in", "concat"] and "[in ch 8..32 of 40][out ch 16..40 of 40]" in lines[1], lines
    sv = R.f16(np.random.default_rng(9).standard_normal((B, OH, OW, 16)))
    g.set(side, sv)
    g.set(xi, x)
    g.compute()
    got = g.get(y)
    np.testing.assert_array_equal(got[..., :16], 2.0 * sv)
    np.testing.assert_array_equal(got[..., 16:].astype(np.float64), want)


# ---- readers of a reshape that changes ne[0] -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("what", ["pool", "conv", "sliced"])
def test_readers_of_a_reshaped_map_fused_against_per_node_and_float64(device, what):
    """x [16 | 32, 4, 4, 2] reshaped to 8 | 16 channels on an 8 x 4 map (space-to-depth by reshape) in front of a max pool, a SiLU conv, and a SiLU conv on
    channels 8..16 of it: the reshaped map is contiguous and its pixels are as wide as the reshape says. Max pool: bit-equal to float64. Conv: the fused run
    rounds once (4 floors against float64), the per-node run twice, the conv's output and then its SiLU, whose slope is at most 1.1 (8 floors); between
    the two that is three roundings of 2^-11 of the largest value at most: 2^-9."""
    rng = np.random.default_rng(len(what))
    cin = 32 if what == "sliced" else 16
    x = R.f16(rng.standard_normal((2, 4, 4, cin)))
    xr = x.reshape(2, 4, 8, cin // 2)
    w = R.f16(rng.standard_normal((8, 3, 3, 8)) / 6)
    if what == "pool":
        want = R.pool2d(xr, R.MAX, 3, 1, 1)
    else:
        src = xr[..., 8:16] if what == "sliced" else xr
        p = np.zeros((2, 6, 10, 8))
        p[:, 1:-1, 1:-1] = src
        want = R.silu(sum(np.einsum("bhwc,oc->bhwo", p[:, ky:ky + 4, kx:kx + 8], w[:, ky, kx]) for ky in range(3) for kx in range(3)))
    got = {}
    for fused in (True, False):
        g = G.Graph(device)
        m = G.ModelRef(g)
        xi = g.input((cin, 4, 4, 2), G.F16, "x")
        r = G.reshape(m, xi, cin // 2, 8, 4, 2)
        if what == "pool":
            y = G.pool_2d(m, r, G.POOL_MAX, 3, 3, 1, 1, 1, 1)
        else:
            g.add_weight("k.weight", w.astype(np.float32), G.F16)
            y = G.silu(m, G.conv_2d(G.ModelRef(g, "k"), G.slice_(m, r, (8, 16)) if what == "sliced" else r, 1, 1))
        g.output(y, "y")
        g.set_fused_models(fused)
        g.allocate()
        lines = g.describe().strip().splitlines()[:-1]
        if fused:
            assert len(lines) == 1 and ("[in ch 8..16 of 16]" in lines[0]) == (what == "sliced"), lines
        g.set(xi, x)
        g.compute()
        got[fused] = g.get(y).astype(np.float64)
        assert got[fused].shape == want.shape
    if what == "pool":
        np.testing.assert_array_equal(got[True], want)
        np.testing.assert_array_equal(got[False], want)
    else:
        floor = R.f16_floor(want)
        e_f, e_n, e_fn = R.rel_err(got[True], want), R.rel_err(got[False], want), R.rel_err(got[True], got[False])
        print(f"silu(conv({what} reshape)): fused {e_f:.3g}, per node {e_n:.3g}, between {e_fn:.3g}; floor {floor:.3g}")
        assert e_f <= 4 * floor and e_n <= 8 * floor and e_fn <= 2.0 ** -9, (e_f, e_n, e_fn, floor)


# ---- SiLU, sub ---------------------------------------------------------------------------------------------------------------------------------------

def _silu_vector():
    x = np.concatenate([[-20.0, -0.0, 11.0, 60000.0, -60000.0, 0.0, 1e-4], np.random.default_rng(2).standard_normal(1001) * 4])
    return R.f16(x)


def _check_silu(got, x, what):
    want = R.silu(x)
    floor = R.f16_floor(want)
    err = R.rel_err(got, want)
    small = np.abs(x) < 100  # the error relative to the largest output says nothing about O(1) values next to 60000
    err_small = R.rel_err(got[small], want[small])
    floor_small = R.f16_floor(want[small])
    print(f"silu {what}: rel err {err:.3g} floor {floor:.3g}; |x| < 100: {err_small:.3g} floor {floor_small:.3g}")
    assert np.isfinite(got).all() and err <= 4 * floor and err_small <= 4 * floor_small


def test_silu_launcher_and_node_against_float64(device):
    x = _silu_vector()
    out = empty(x.size * 2, zero=False)
    L.vx_check(api().vx_unary_f16(4, dev(_h(x)).ptr, out.ptr, x.size, 0.0, None))
    sync()
    _check_silu(out.to_numpy(np.float16, x.shape).astype(np.float64), x, "launcher")
    g = G.Graph(device)
    xi = g.input((x.size,), G.F16, "x")
    y = g.output(G.silu(G.ModelRef(g), xi), "y")
    g.allocate()
    assert g.describe().strip().splitlines()[:-1] == [f"silu n={x.size}"]
    g.set(xi, x)
    g.compute()
    _check_silu(g.get(y).ravel().astype(np.float64), x, "node")
    assert api().vx_unary_f16(5, out.ptr, out.ptr, 8, 0.0, None) == 0 and b"4 silu" in api().vx_last_error()


def test_sub_launcher_and_node(device):
    rng = np.random.default_rng(3)
    a, b = R.f16(rng.standard_normal((5, 7, 24))), R.f16(rng.standard_normal(24))
    want = a - b
    out = empty(a.size * 2, zero=False)
    L.vx_check(api().vx_binary_rows(2, dev(_h(a)).ptr, 0, dev(_h(b)).ptr, 0, 24, out.ptr, 0, a.size, None))
    sync()
    np.testing.assert_array_equal(out.to_numpy(np.float16, a.shape), _h(want))  # one rounding of an exact f32 difference
    g = G.Graph(device)
    m = G.ModelRef(g)
    ai, bi = g.input((24, 7, 5), G.F16, "a"), g.input((24,), G.F16, "b")
    y = g.output(G.sub(m, ai, bi), "y")
    g.allocate()
    assert g.describe().strip().splitlines()[:-1] == ["sub n=840 period=24"]
    g.set(ai, a)
    g.set(bi, b)
    g.compute()
    np.testing.assert_array_equal(_h(g.get(y)).reshape(want.shape), _h(want))
    assert api().vx_binary_rows(3, out.ptr, 0, out.ptr, 0, 8, out.ptr, 0, 8, None) == 0 and b"2 sub" in api().vx_last_error()


# ---- softmax, softmax expectation, row sums ------------------------------------------------------------------------------------------------------------

SOFTMAX_CASES = [(16, 4 * 37), (8, 5), (80, 3), (1024, 2)]  # (n, rows): one thread per row at 8 and 16, one wave per row above (two chunks per lane at 1024)


def _softmax_rows(n, rows):
    x = R.f16(np.random.default_rng(n + rows).standard_normal((rows, n)) * 3)
    x[0] = R.f16(np.linspace(-60000, 60000, n))  # logits at the f16 limit
    x[1] = 3.5                                   # all equal
    return x


@pytest.mark.parametrize("n,rows", SOFTMAX_CASES)
def test_softmax_rows_launcher_and_node_against_float64(device, n, rows):
    x = _softmax_rows(n, rows)
    want = R.softmax(x)
    floor = R.f16_floor(want)
    out = empty(x.size * 2, zero=False)
    L.vx_check(api().vx_softmax_rows_f16(dev(_h(x)).ptr, n, out.ptr, n, rows, n, None))
    sync()
    got = out.to_numpy(np.float16, x.shape).astype(np.float64)
    g = G.Graph(device)
    xi = g.input((n, rows), G.F16, "x")
    y = g.output(G.soft_max(G.ModelRef(g), xi), "y")
    g.allocate()
    assert g.describe().strip().splitlines()[:-1] == [f"soft_max rows={rows} n={n}"]
    g.set(xi, x)
    g.compute()
    node = g.get(y).reshape(x.shape).astype(np.float64)
    for what, v in (("launcher", got), ("node", node)):
        err = R.rel_err(v, want)
        print(f"softmax n={n} rows={rows} {what}: rel err {err:.3g} floor {floor:.3g} bound {4 * floor:.3g}")
        assert np.isfinite(v).all() and err <= 4 * floor, (n, rows, what, err, floor)
        np.testing.assert_allclose(v[1], 1.0 / n, rtol=2.0 ** -10)
    np.testing.assert_array_equal(got, node)


def test_softmax_rows_launcher_refusals():
    b = empty(4096)
    for n in (12, 1032, 0):
        assert api().vx_softmax_rows_f16(b.ptr, 1032, b.ptr, 1032, 1, n, None) == 0 and b"vx_softmax_rows_f16" in api().vx_last_error()
    assert api().vx_softmax_rows_f16(b.ptr, 8, b.ptr, 16, 2, 16, None) == 0 and b"row strides" in api().vx_last_error()


def _expect_case():
    """37 rows of 64 + 16 channels: 4 groups of 16 box logits, then 16 channels the launch must not read"""
    rng = np.random.default_rng(7)
    x = R.f16(rng.standard_normal((37, 80)) * 4)
    x[0, :16] = R.f16(np.linspace(-60000, 60000, 16))
    x[1, 16:32] = -2.25
    x[:, 64:] = 60000.0
    proj = np.arange(16, dtype=np.float32)
    return x, proj, R.softmax_expect(x[:, :64].reshape(37, 4, 16), proj)


def test_softmax_expect_launcher_against_float64():
    x, proj, want = _expect_case()
    floor = R.f16_floor(want)
    out = empty(want.size * 2, zero=False)
    L.vx_check(api().vx_softmax_expect_f16(dev(_h(x)).ptr, 80, 4, dev(proj).ptr, out.ptr, 37, 16, None))
    sync()
    got = out.to_numpy(np.float16, want.shape).astype(np.float64)
    err = R.rel_err(got, want)
    print(f"softmax_expect launcher: rel err {err:.3g} floor {floor:.3g} bound {4 * floor:.3g}")
    assert np.isfinite(got).all() and err <= 4 * floor and abs(got[1, 1] - 7.5) < 1e-2
    assert api().vx_softmax_expect_f16(out.ptr, 56, 4, out.ptr, out.ptr, 1, 16, None) == 0 and b"row stride" in api().vx_last_error()


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "per_node"])
def test_dfl_chain_against_float64(device, fused):
    """slice -> reshape -> soft_max -> mul -> sum_rows on two images. One launch: the floor rule. Per node every term meets three f16 roundings (the
    softmax, the product, the sum: 2^-11 each) on top of the softmax kernel's own 4 floors, 7 x 2^-11 of the largest output in all: bound 2^-8."""
    x, proj, want = _expect_case()
    x2 = np.stack([x, x[::-1]])  # [N = 2, A = 37, 80]
    want2 = np.stack([want, want[::-1]])
    g = G.Graph(device)
    m = G.ModelRef(g)
    xi = g.input((80, 37, 1, 2), G.F16, "x")
    p = g.add_weight("proj", proj, G.F32)
    y = g.output(G.yolo_dfl_forward(m, p, G.cont(m, G.slice_(m, xi, (0, 64))), 16), "y")
    g.set_fused_models(fused)
    g.allocate()
    lines = g.describe().strip().splitlines()[:-1]
    assert (lines == ["softmax_expect rows=74 groups=4 n=16 [in ch 0..64 of 80]"]) if fused else ([l.split()[0] for l in lines] == ["slice", "soft_max", "mul", "sum_rows"]), lines
    g.set(xi, x2)
    g.compute()
    got = g.get(y).reshape(2, 37, 4).astype(np.float64)
    err, floor = R.rel_err(got, want2), R.f16_floor(want2)
    print(f"dfl chain {'fused' if fused else 'per node'}: rel err {err:.3g} floor {floor:.3g}")
    assert np.isfinite(got).all() and err <= (4 * floor if fused else 2.0 ** -8), (err, floor)


def test_sum_rows_launcher_and_node_against_float64(device):
    x = R.f16(np.random.default_rng(8).standard_normal((3, 37, 20)))
    want = R.sum_rows(x)
    floor = R.f16_floor(want)
    out = empty(want.size * 2, zero=False)
    L.vx_check(api().vx_sum_rows_f16(dev(_h(x)).ptr, out.ptr, 3 * 37, 20, None))
    sync()
    got = out.to_numpy(np.float16, want.shape).astype(np.float64)
    g = G.Graph(device)
    xi = g.input((20, 37, 3), G.F16, "x")
    y = g.output(G.sum_rows(G.ModelRef(g), xi), "y")
    g.allocate()
    assert g.describe().strip().splitlines()[:-1] == ["sum_rows rows=111 n=20"]
    g.set(xi, x)
    g.compute()
    node = g.get(y).reshape(want.shape).astype(np.float64)
    err = R.rel_err(got, want)
    print(f"sum_rows: rel err {err:.3g} floor {floor:.3g}")
    assert err <= 4 * floor
    np.testing.assert_array_equal(got, node)


# ---- the blocks ----------------------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def net(tmp_path_factory):
    """the detector's file, its f16-rounded weights, two images, and the reference's outputs for them (computed once, read-only)"""
    sd = synth.yolov9t_state_dict(0)
    path = synth.write_yolov9t_gguf(tmp_path_factory.mktemp("yolo") / "y0.gguf", sd=sd)
    W = Y.f16_rounded(sd)
    x = synth.images(2, 96, 96, seed=96).astype(np.float32) / np.float32(255.0)
    wb, ws, feats, raws = Y.forward(W, x, return_features=True)
    for a in (x, wb, ws, *feats.values(), *raws):
        a.setflags(write=False)
    return dict(path=path, W=W, x=x, boxes=wb, scores=ws, feats=feats, raws=raws)


BLOCKS = {
    "elan1": (32, 12, 9, lambda m, x: G.yolo_elan1(m, x, "model.2", 32, 32, 32, 16), lambda W, x: Y.elan1(W, "model.2", x)),
    "rep_ncsp_elan4": (64, 12, 9, lambda m, x: G.yolo_rep_ncsp_elan4(m, x, "model.4", 64, 64, 64, 32, 3), lambda W, x: Y.repncspelan4(W, "model.4", x)),
    "sppelan": (128, 3, 3, lambda m, x: G.yolo_sppelan(m, x, "model.9", 128, 128, 64), lambda W, x: Y.sppelan(W, "model.9", x)),
    "aconv": (32, 12, 9, lambda m, x: G.yolo_aconv(m, x, "model.3"), lambda W, x: Y.aconv(W, "model.3", x)),
}
_block_want = {}


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "per_node"])
@pytest.mark.parametrize("name", list(BLOCKS))
def test_block_against_the_reference(device, net, name, fused):
    C, w, h, build, ref = BLOCKS[name]
    if name not in _block_want:
        x = R.f16(np.random.default_rng(len(name)).standard_normal((2, h, w, C))).astype(np.float32)
        want = ref(net["W"], x)
        want.setflags(write=False)
        _block_want[name] = (x, want)
    x, want = _block_want[name]
    g = G.Graph(device, G.Weights(net["path"]))
    xi = g.input((C, w, h, 2), G.F16, "x")
    y = g.output(build(G.ModelRef(g), xi), "y")
    g.set_fused_models(fused)
    g.allocate()
    g.set(xi, x)
    g.compute()
    got = g.get(y)
    assert got.shape == want.shape and np.isfinite(got).all()
    err = R.rel_err(got, want)
    print(f"block {name} {'fused' if fused else 'per node'}: rel err {err:.3g} (largest value {np.abs(want).max():.3g}); bound 2e-2")
    assert err < 2e-2, (name, fused, err)


# ---- the whole network ---------------------------------------------------------------------------------------------------------------------------------

FEATURES = (2, 4, 9, 15, 21)


def _network(device, net, fused, batch):
    g = G.Graph(device, G.Weights(net["path"]))
    image = g.input((3, 96, 96, batch), G.F32, "image")
    boxes, scores, raw, f = G.yolov9t_forward(G.ModelRef(g), image)
    outs = dict(boxes=g.output(boxes, "boxes"), scores=g.output(scores, "scores"))
    outs.update({f"raw{i}": g.output(r, f"raw{i}") for i, r in enumerate(raw)})
    outs.update({f"f{k}": g.output(f[k], f"f{k}") for k in FEATURES})
    g.set_fused_models(fused)
    g.use_hip_graph(True)
    g.allocate()
    return g, image, outs


def _read(g, outs, batch):
    got = {k: g.get(t) for k, t in outs.items()}
    got["boxes"] = got["boxes"].reshape(batch, -1, 4)
    got["scores"] = got["scores"].reshape(batch, -1, got["scores"].shape[-1])
    return got


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "per_node"])
def test_network_against_the_reference(device, net, fused):
    g, image, outs = _network(device, net, fused, 2)
    g.set(image, net["x"])
    g.compute()
    got = _read(g, outs, 2)
    tag = "fused" if fused else "per node"
    for k in FEATURES:
        want = net["feats"][k]
        assert got[f"f{k}"].shape == want.shape, k
        err = R.rel_err(got[f"f{k}"], want)
        print(f"{tag} feature {k}: rel err {err:.3g}; bound 2e-2")
        assert err < 2e-2, (k, err)
    for i, want in enumerate(net["raws"]):
        assert got[f"raw{i}"].shape == want.shape, i
        err = float(np.abs(got[f"raw{i}"] - want).max())
        print(f"{tag} raw map {i}: max abs err {err:.3g}; bound 5e-2")
        assert err < 5e-2, (i, err)
    e_s, e_b = float(np.abs(got["scores"] - net["scores"]).max()), float(np.abs(got["boxes"] - net["boxes"]).max())
    print(f"{tag}: scores max abs {e_s:.2e} (bound {SCORE_TOL}), boxes max abs {e_b:.3f} px (bound {BOX_TOL})")
    assert e_s <= SCORE_TOL and e_b <= BOX_TOL
    # the second compute replays the launch list as one hipGraph: bit-identical
    g.compute()
    again = _read(g, outs, 2)
    for k in got:
        np.testing.assert_array_equal(again[k], got[k], err_msg=k)
    # image 0 encoded alone gives the bits it gives in the batch
    g1, image1, outs1 = _network(device, net, fused, 1)
    g1.set(image1, net["x"][:1])
    g1.compute()
    alone = _read(g1, outs1, 1)
    for k in got:
        np.testing.assert_array_equal(alone[k][0], got[k][0], err_msg=k)


def test_network_without_feature_outputs_gives_the_same_bits(device, net):
    """The graph a user builds -- boxes, scores and raw maps as the only outputs -- is the 212-launch list in which model.4 and model.9 are written into
    their concats too and the first upsample reads model.9 there (a graph output is never placed, so the runs above copy those two: 214 launches).
    Where a map lies changes no arithmetic: every output equals the feature-output run bit for bit, and meets the same bounds against the reference."""
    ga, image_a, outs_a = _network(device, net, True, 2)
    g = G.Graph(device, G.Weights(net["path"]))
    image = g.input((3, 96, 96, 2), G.F32, "image")
    boxes, scores, raw, _ = G.yolov9t_forward(G.ModelRef(g), image)
    outs = dict(boxes=g.output(boxes, "boxes"), scores=g.output(scores, "scores"), **{f"raw{i}": g.output(r, f"raw{i}") for i, r in enumerate(raw)})
    g.use_hip_graph(True)
    g.allocate()
    lines = g.describe().strip().splitlines()[:-1]
    assert len(lines) == 212 and ga.summary()["launches"] == 214
    assert "nearest[in ch 64..192 of 192][out ch 0..128 of 224] 3x3 -> 6x6 C=128" in lines and not [l for l in lines if l.startswith("concat part") and "[144," not in l and "[2," not in l], lines
    ga.set(image_a, net["x"])
    ga.compute()
    want = _read(ga, outs_a, 2)
    g.set(image, net["x"])
    for _ in range(2):  # direct, then the hipGraph replay
        g.compute()
        got = _read(g, outs, 2)
        for k in got:
            np.testing.assert_array_equal(got[k], want[k], err_msg=k)
    e_s, e_b = float(np.abs(got["scores"] - net["scores"]).max()), float(np.abs(got["boxes"] - net["boxes"]).max())
    assert e_s <= SCORE_TOL and e_b <= BOX_TOL and all(float(np.abs(got[f"raw{i}"] - r).max()) < 5e-2 for i, r in enumerate(net["raws"]))


def test_network_scores_against_the_hand_schedule(device, net):
    """vision.Yolov9t.forward on the same file: both fold the RepConv's 1x1 into the 3x3 and round alike, but the launch lists differ, so SCORE_TOL, not bits"""
    model = vision.Yolov9t.load(net["path"], device)
    hb, hs = model.forward(np.asarray(net["x"]))
    g, image, outs = _network(device, net, True, 2)
    g.set(image, net["x"])
    g.compute()
    got = _read(g, outs, 2)
    e_s, e_b = float(np.abs(got["scores"] - hs).max()), float(np.abs(got["boxes"] - hb).max())
    print(f"graph vs hand schedule: scores max abs {e_s:.2e}, boxes max abs {e_b:.3f} px")
    assert e_s <= SCORE_TOL and e_b <= BOX_TOL

"""-m gpu: the graph layer's MI-GAN kernels (vx_clamp_f16, vx_binary_plane_f16 in csrc/kernels_graph.hip; vx_upfirdn2x_f16, vx_dwconv_agc_f16 in
csrc/kernels_fir.hip), each directly and through its node or fused group, and MI-GAN built through vision.cpp_amd/graph.py::migan_generate -- against
float64 numpy on f16-rounded operands (tests/fir_ref.py) and against tests/migan_ref.py's restatement of src/visp/arch/migan.cpp on f16-rounded weights,
block by block and as a whole, fused and per node, and against the hand schedule of csrc/migan.cpp.

Bounds. Clamp is bit-equal to float64: a clamp of f16 values to f16-representable bounds is one of them or a bound. The plane ops, the FIR upsample and the
depthwise conv with lrelu_agc are within 4 x the floor, the floor being the float64 result rounded to f16 against itself (the rule of DESIGN.md section 14):
their f32 arithmetic (at most 16 products) is far below one f16 rounding. Blocks and network, fused: FUSED_TOL = 5e-3 absolute -- the project's bound for the
hand schedule, whose arithmetic the fused path does. Per node every op rounds to f16 once more: PER_NODE_TOL is four times the largest
error of a per-node run against migan_ref measured on MI355X (below), taken over max(1, largest value), and must stay under 2e-2, section 17's block bound. A fused
run against a per-node run of the same graph: each is within its bound of the reference, so the two are within FUSED_TOL + PER_NODE_TOL of each other.

Measured on MI355X (DESIGN.md section 18 has all of it): clamp bit-equal; every plane, FIR upsample (launcher and fused group) and dwconv_agc case equal to
its floor (1.7e-4 .. 4.8e-4); the FIR group per node at most 9.7e-4. Blocks fused / per node, error over max(1, largest value): separable conv plain 3.9e-4 /
5.5e-4, down 4.5e-4 / 4.6e-4, up + noise 4.1e-4 / 6.5e-4, noise 5.8e-4 / 7.5e-4; synthesis block x 3.9e-4 / 6.0e-4, image 5.4e-4 / 5.4e-4. Generator: res 16
1.8e-4 / 3.0e-4, res 32 7.8e-4 / 1.10e-3 (outputs up to 0.64) -- 1.10e-3 is the largest per-node figure, so PER_NODE_TOL = 4.4e-3. With a changed filter_const, against
migan_ref on the same weights: 1.10e-3 per node, 1.17e-3 for the fused graph whose one group stays per node (held to the per-node bound); 1.22e-3 between the two. 64-wide at res 32: graph 2.9e-4 and hand schedule 3.5e-4 from the reference, 4.4e-4 from each other."""
import numpy as np
import pytest

import fir_ref as R
import migan_ref
from visioncpp_amd import _lib as L
from visioncpp_amd import graph as G
from visioncpp_amd import synth, vision

pytestmark = pytest.mark.gpu

from gpu_util import api, dev, empty, release, sync  # noqa: E402

FUSED_TOL = 5e-3
# largest error of a per-node run against migan_ref, over max(1, largest value), measured on MI355X over the blocks and networks of this file; the bound is four times that
PER_NODE_MEASURED = 1.10e-3
PER_NODE_TOL = 4 * PER_NODE_MEASURED
assert PER_NODE_TOL <= 2e-2
SQRT2 = float(np.float32(1.4142135623))
CH = dict(ch_base=256, ch_max=24)


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


def _lines(g):
    return g.describe().strip().splitlines()[:-1]


def _within_floors(got, want, what):
    floor = R.f16_floor(want)
    err = R.rel_err(got, want)
    print(f"{what}: rel err {err:.3g} floor {floor:.3g} bound {4 * floor:.3g}")
    assert np.isfinite(np.asarray(got, np.float32)).all() and err <= 4 * floor, (what, err, floor)


# ---- clamp ------------------------------------------------------------------------------------------------------------------------------------------

def _clamp_values():
    v = np.concatenate([R.f16(np.random.default_rng(0).standard_normal(998) * 300), [60000.0, -60000.0, 256.0, -256.0, 255.9, -255.9, 0.0, -0.0, np.inf, -np.inf]])
    assert v.size == 1008
    return R.f16(v)


def test_clamp_launcher_and_node_are_bit_equal(device):
    v = _clamp_values()
    want = R.clamp(v, -256.0, 256.0)
    out = empty(v.size * 2, zero=False)
    L.vx_check(api().vx_clamp_f16(dev(_h(v)).ptr, out.ptr, v.size, -256.0, 256.0, None))
    sync()
    got = out.to_numpy(np.float16, v.shape)
    np.testing.assert_array_equal(got.astype(np.float64), want)
    assert np.signbit(got[-3]) and (np.abs(got.astype(np.float64)) > 256).sum() == 0 and (np.abs(v) > 256).sum() > 100
    g = G.Graph(device)
    x = g.input((v.size,), G.F16, "x")
    y = g.output(G.clamp(G.ModelRef(g), x, -256.0, 256.0), "y")
    g.allocate()
    assert _lines(g) == ["clamp n=1008"]
    g.set(x, v)
    g.compute()
    np.testing.assert_array_equal(g.get(y).ravel().astype(np.float64), want)
    assert api().vx_clamp_f16(out.ptr, out.ptr, 8, 1.0, -1.0, None) == 0 and b"bounds" in api().vx_last_error()


# ---- plane broadcast ----------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [(2, 3, 5, 8), (1, 4, 4, 24)])
@pytest.mark.parametrize("b_f32", [0, 1])
def test_plane_launcher_and_node(device, shape, b_f32):
    B, H, W, C = shape
    rng = np.random.default_rng(B * 100 + C + b_f32)
    a = R.f16(rng.standard_normal(shape) * 3)
    b = rng.standard_normal((H, W)) * 2
    b = b.astype(np.float32).astype(np.float64) if b_f32 else R.f16(b)
    ad = dev(_h(a))
    bd = dev(b.astype(np.float32) if b_f32 else _h(b))
    for op, fn in ((R.ADD, G.add), (R.MUL, G.mul), (R.SUB, G.sub)):
        want = R.plane_binary(op, a, b)
        out = empty(a.size * 2, zero=False)
        L.vx_check(api().vx_binary_plane_f16(op, ad.ptr, bd.ptr, b_f32, out.ptr, B, H * W, C, None))
        sync()
        _within_floors(out.to_numpy(np.float16, shape), want, f"plane launcher op {op} {shape} b_f32={b_f32}")
        g = G.Graph(device)
        m = G.ModelRef(g)
        x = g.input((C, W, H, B), G.F16, "x")
        # a constant of either type is read as f32; an activation plane as f16
        p = g.add_weight("p", b.reshape(1, H, W, 1), G.F32) if b_f32 else g.input((1, W, H, 1), G.F16, "p")
        y = g.output(fn(m, x, p), "y")
        g.allocate()
        assert _lines(g) == [f"{['add', 'mul', 'sub'][op]}_plane B={B} HW={H * W} C={C}{' (constant)' if b_f32 else ''}"]
        g.set(x, a)
        if not b_f32:
            g.set(p, b)
        g.compute()
        _within_floors(_h(g.get(y)), want, f"plane node op {op} {shape} b_f32={b_f32}")
    assert api().vx_binary_plane_f16(0, ad.ptr, bd.ptr, b_f32, ad.ptr, B, H * W, 12, None) == 0 and b"multiple of 8" in api().vx_last_error()


# ---- the 4-channel f32 image ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [1, 3])
def test_image4_pad8_and_the_conv_on_a_four_channel_image(device, k):
    rng = np.random.default_rng(40 + k)
    img = rng.uniform(-1, 1, (2, 7, 9, 4)).astype(np.float32)
    out = empty(img.size // 4 * 16, zero=False)
    L.vx_check(api().vx_image4_pad8_f32(dev(img).ptr, out.ptr, img.size // 4, None))
    sync()
    got = out.to_numpy(np.float16, (2, 7, 9, 8))
    hi = img.astype(np.float16)
    np.testing.assert_array_equal(got[..., :4], hi)  # the values rounded to f16, and what the rounding dropped, rounded itself
    np.testing.assert_array_equal(got[..., 4:], (img - hi.astype(np.float32)).astype(np.float16))
    w = R.f16(rng.standard_normal((16, k, k, 4)) / 2)  # numpy order of ne [4, k, k, 16]
    bias = (rng.standard_normal(16) * 0.05).astype(np.float32)
    g = G.Graph(device)
    m = G.ModelRef(g)
    g.add_weight("c.weight", w, G.F16)
    g.add_weight("c.bias", bias, G.F32)
    xi = g.input((4, 9, 7, 2), G.F32, "image")
    y = g.output(G.conv_2d(m["c"], xi, 1, k // 2), "y")
    g.allocate()
    assert _lines(g)[0] == "image4_pad8 [4, 9, 7, 2]" and len(_lines(g)) == 2
    g.set(xi, img)
    g.compute()
    # the conv sees the f32 image up to the residue's own rounding (below 2^-22 here): float64 on the f32 pixels
    pad = k // 2
    p = np.zeros((2, 7 + 2 * pad, 9 + 2 * pad, 4))
    p[:, pad:pad + 7, pad:pad + 9] = img
    want = sum(np.einsum("bhwc,oc->bhwo", p[:, i:i + 7, j:j + 9], w[:, i, j]) for i in range(k) for j in range(k)) + bias
    _within_floors(_h(g.get(y)), want, f"conv{k}x{k} on the 4-channel image")


# ---- vx_upfirdn2x_f16 ---------------------------------------------------------------------------------------------------------------------------------

# (B, h, w, C), plane, agc, res: every tap at a border; non-square with an odd width; a channel slice into a slice of a wider buffer (direct only); the whole
# epilogue; a residual alone; then, on a filter with f[ky][kx] != f[kx][ky] != f[3 - ky][3 - kx] (fir_ref.asymmetric_fir: the symmetric filter of the cases
# before hides flipped, transposed and mispaired taps): bare, and the whole epilogue
UP_CASES = [((2, 1, 1, 8), False, False, False), ((1, 2, 3, 24), False, False, False), ((1, 5, 9, 16), False, False, False), ((2, 4, 4, 8), True, True, True),
            ((1, 3, 4, 8), False, False, True), ((1, 2, 3, 24), False, False, False), ((2, 4, 4, 8), True, True, True)]
SLICE_CASE = 2
ASYMMETRIC_CASES = (5, 6)
_up_cache = {}


def _up_case(i):
    if i not in _up_cache:
        (B, h, w, C), plane, agc, res = UP_CASES[i]
        rng = np.random.default_rng(700 + i)
        x = R.f16(rng.standard_normal((B, h, w, 32 if i == SLICE_CASE else C)) * (400.0 if agc else 1.0))
        fir = R.f16((R.asymmetric_fir if i in ASYMMETRIC_CASES else R.perturbed_fir)(rng, C))
        pl = rng.standard_normal((2 * h, 2 * w)).astype(np.float32).astype(np.float64) if plane else None
        rs = R.f16(rng.standard_normal((B, 2 * h, 2 * w, C)) * 2) if res else None
        a = (SQRT2, 256.0) if agc else None
        want = R.upfirdn2x(x[..., 8:24] if i == SLICE_CASE else x, fir, pl, rs, a)
        if agc:  # the clamp acts on a share of the values that is neither negligible nor all of them, in the reference itself
            frac = R.clamped_fraction(x, fir, pl, a)
            assert 0.01 <= frac <= 0.5, frac
        for arr in (x, fir, want):
            arr.setflags(write=False)
        _up_cache[i] = (x, fir, pl, rs, a, want)
    return _up_cache[i]


@pytest.mark.parametrize("i", range(len(UP_CASES)))
def test_upfirdn_launcher_against_float64(i):
    (B, h, w, C), *_ = UP_CASES[i]
    x, fir, pl, rs, a, want = _up_case(i)
    xd, fd = dev(_h(x)), dev(_h(fir.reshape(16, C)))
    pd = dev(pl.astype(np.float32)) if pl is not None else None
    rd = dev(_h(rs)) if rs is not None else None
    args = (pd.ptr if pd else None, rd.ptr if rd else None, C, int(a is not None), a[0] if a else 1.0, a[1] if a else 0.0, B, h, w, C, None)
    if i == SLICE_CASE:
        out = dev(np.full((B, 2 * h, 2 * w, 40), 7.0, np.float16))
        L.vx_check(api().vx_upfirdn2x_f16(xd.ptr + 8 * 2, 32, fd.ptr, out.ptr + 16 * 2, 40, *args))
        sync()
        full = out.to_numpy(np.float16, (B, 2 * h, 2 * w, 40))
        assert (full[..., :16] == 7.0).all() and (full[..., 32:] == 7.0).all(), "the buffer outside the written slice was touched"
        got = full[..., 16:32]
    else:
        out = empty(want.size * 2, zero=False)
        L.vx_check(api().vx_upfirdn2x_f16(xd.ptr, C, fd.ptr, out.ptr, C, *args))
        sync()
        got = out.to_numpy(np.float16, want.shape)
    _within_floors(got, want, f"upfirdn launcher {UP_CASES[i]}")


def test_upfirdn_launcher_refuses_what_it_was_not_built_for():
    x = dev(np.zeros((1, 2, 2, 16), np.float16))
    f = dev(np.zeros((16, 16), np.float16))
    y = empty(4 * 4 * 16 * 2)
    for (x_pix, y_pix, res, res_pix, agc, clamp_, C), msg in [((16, 16, None, 0, 0, 0.0, 12), b"multiple of 8"), ((8, 16, None, 0, 0, 0.0, 16), b"pixel strides"),
                                                             ((16, 20, None, 0, 0, 0.0, 16), b"pixel strides"), ((16, 16, y.ptr + 2, 16, 0, 0.0, 16), b"16-byte aligned"),
                                                             ((16, 16, x.ptr, 8, 0, 0.0, 16), b"residual pixel stride"), ((16, 16, None, 0, 1, -1.0, 16), b"clamp"),
                                                             ((16, 16, y.ptr, 16, 0, 0.0, 16), b"alias"), ((16, 16, y.ptr + 16, 32, 0, 0.0, 16), b"overlap")]:
        assert api().vx_upfirdn2x_f16(x.ptr, x_pix, f.ptr, y.ptr, y_pix, None, res, res_pix, agc, 1.0, clamp_, 1, 2, 2, C, None) == 0 and msg in api().vx_last_error(), msg


@pytest.mark.parametrize("i", [j for j in range(len(UP_CASES)) if j != SLICE_CASE])
@pytest.mark.parametrize("fused", [True, False])
def test_upfirdn_group_against_float64(device, i, fused):
    (B, h, w, C), plane, agc, res = UP_CASES[i]
    x, fir, pl, rs, a, want = _up_case(i)
    g = G.Graph(device)
    g.set_fused_models(fused)
    m = G.ModelRef(g)
    g.add_weight("up.filter_const", np.tile(np.array([[1.0, 0.0], [0.0, 0.0]], np.float32), (h, w))[None, None], G.F16)
    g.add_weight("up.filter.weight", fir.transpose(2, 0, 1)[..., None], G.F16)  # ne [1, 4, 4, C]
    xi = g.input((C, w, h, B), G.F16, "x")
    t = G.migan_upsample_2d(m["up"], xi)
    if plane:
        t = G.add(m, t, g.add_weight("noise", pl.reshape(1, 2 * h, 2 * w, 1), G.F32))
    if agc:
        t = G.migan_lrelu_agc(m, t, 0.2, SQRT2, 256)
    ri = g.input((C, 2 * w, 2 * h, B), G.F16, "res") if res else None
    if res:
        t = G.add(m, t, ri)
    y = g.output(t, "y")
    g.allocate()
    lines = _lines(g)
    if fused:
        assert len(lines) == 1 and lines[0].startswith("upfirdn2x" + ("[+plane]" if plane else "") + ("[lrelu_agc 0.2 1.41421 256]" if agc else "") + ("[+res]" if res else "") + " B="), lines
    else:
        assert [l.split()[0] for l in lines[:4]] == ["nearest", "mul_plane", "dwconv4x4", "slice"] and len(lines) == 4 + plane + 3 * agc + res, lines
    g.set(xi, x)
    if res:
        g.set(ri, rs)
    g.compute()
    got = _h(g.get(y))
    if fused:
        _within_floors(got, want, f"upfirdn group {UP_CASES[i]}")
    else:  # one f16 rounding per node: within the per-node bound of the largest value
        err = R.rel_err(got, want)
        print(f"upfirdn per node {UP_CASES[i]}: rel err {err:.3g}")
        assert err <= PER_NODE_TOL


# ---- vx_dwconv_agc_f16 ----------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", [(3, 1, 1, 8, 3, 3, 2), (3, 1, 1, 24, 5, 7, 1)])
def test_dwconv_agc_launcher_and_group(device, case):
    k, s, pad, C, H, W, B = case
    rng = np.random.default_rng(sum(case))
    x = R.f16(rng.standard_normal((B, H, W, C)) * 250)
    w = R.f16(rng.standard_normal((k, k, C)) / 3)
    bias = (rng.standard_normal(C) * 0.05).astype(np.float32).astype(np.float64)
    pre = R.lrelu_agc(R.depthwise(x, w, bias, s, pad), 0.2, SQRT2, 0.0)
    frac = float((np.abs(pre) > 256).mean())
    assert 0.01 <= frac <= 0.5, frac
    want = R.lrelu_agc(R.depthwise(x, w, bias, s, pad), 0.2, SQRT2, 256.0)
    out = empty(want.size * 2, zero=False)
    L.vx_check(api().vx_dwconv_agc_f16(dev(_h(x)).ptr, dev(_h(w.reshape(k * k, C))).ptr, dev(bias.astype(np.float32)).ptr, out.ptr, B, H, W, C, k, s, pad, 0.2, SQRT2, 256.0, None))
    sync()
    _within_floors(out.to_numpy(np.float16, want.shape), want, f"dwconv_agc launcher {case}")
    g = G.Graph(device)
    m = G.ModelRef(g)
    g.add_weight("dw.weight", w.transpose(2, 0, 1)[..., None], G.F16)
    g.add_weight("dw.bias", bias, G.F32)
    xi = g.input((C, W, H, B), G.F16, "x")
    y = g.output(G.migan_lrelu_agc(m, G.conv_2d_depthwise(m["dw"], xi, s, pad), 0.2, SQRT2, 256), "y")
    g.allocate()
    lines = _lines(g)
    assert len(lines) == 1 and lines[0].startswith("dwconv3x3[lrelu_agc 0.2 1.41421 256] "), lines
    g.set(xi, x)
    g.compute()
    _within_floors(_h(g.get(y)), want, f"dwconv_agc group {case}")
    assert api().vx_dwconv_agc_f16(out.ptr, out.ptr, None, out.ptr, 1, 3, 3, 8, 3, 1, 1, 0.2, 1.0, -1.0, None) == 0 and b"clamp" in api().vx_last_error()


# ---- blocks against migan_ref ---------------------------------------------------------------------------------------------------------------------------

H0, W0, NB = 4, 6, 2  # a 6 x 4 map, batch 2


def _sep_sd(rng, sd, p, cin, cout, H, W, down=False, up=False, noise=False):
    """the tensors of one separable_conv_2d whose OUTPUT is H x W, with torch names and shapes (synth.migan_state_dict's, for a map that is not square)"""
    sd[f"{p}.conv1.weight"] = (rng.standard_normal((cin, 1, 3, 3)) / 3.0).astype(np.float32)
    sd[f"{p}.conv1.bias"] = (rng.standard_normal(cin) * 0.05).astype(np.float32)
    sd[f"{p}.conv2.weight"] = (rng.standard_normal((cout, cin, 1, 1)) / np.sqrt(cin)).astype(np.float32)
    if down:
        sd[f"{p}.downsample.filter.weight"] = synth._migan_fir(rng, cin, 1.0)
    if up:
        sd[f"{p}.upsample.filter_const"] = np.tile(np.array([[1.0, 0.0], [0.0, 0.0]], np.float32), (H // 2, W // 2))[None, None]
        sd[f"{p}.upsample.filter.weight"] = synth._migan_fir(rng, cout, 4.0)
    if noise:
        sd[f"{p}.noise_const"] = rng.standard_normal((H, W)).astype(np.float32)
        sd[f"{p}.noise_strength"] = np.array([rng.uniform(0.05, 0.2)], np.float32)


def _close(got, want, fused, what):
    scale = 1.0 if fused is True else max(1.0, float(np.abs(want).max()))  # the fused bound is absolute
    err = float(np.abs(np.asarray(got, np.float64) - want).max()) / scale
    tol = {True: FUSED_TOL, False: PER_NODE_TOL, "both": FUSED_TOL + PER_NODE_TOL}[fused]
    print(f"{what} {'fused' if fused is True else ('per node' if fused is False else 'fused against per node')}: max abs err{'' if fused is True else ' / max(1, largest)'} {err:.3g} "
          f"(largest {np.abs(want).max():.3g}) bound {tol:.3g}")
    assert np.isfinite(got).all() and err <= tol, (what, fused, err)
    return err


_block_cache = {}


def _block_weights(tmp_path_factory):
    if "sd" not in _block_cache:
        rng = np.random.default_rng(77)
        sd = {}
        _sep_sd(rng, sd, "plain", 16, 24, H0, W0)
        _sep_sd(rng, sd, "down", 16, 24, H0 // 2, W0 // 2, down=True)
        _sep_sd(rng, sd, "upn", 16, 24, 2 * H0, 2 * W0, up=True, noise=True)
        _sep_sd(rng, sd, "noise", 16, 24, H0, W0, noise=True)
        _sep_sd(rng, sd, "blk.conv1", 16, 24, 2 * H0, 2 * W0, up=True, noise=True)
        _sep_sd(rng, sd, "blk.conv2", 24, 24, 2 * H0, 2 * W0, noise=True)
        sd["blk.torgb.weight"] = (rng.standard_normal((3, 24, 1, 1)) * 0.12 / np.sqrt(24)).astype(np.float32)
        sd["blk.torgb.bias"] = (rng.standard_normal(3) * 0.02).astype(np.float32)
        sd["blk.upsample.filter_const"] = np.tile(np.array([[1.0, 0.0], [0.0, 0.0]], np.float32), (H0, W0))[None, None]
        sd["blk.upsample.filter.weight"] = synth._migan_fir(rng, 3, 4.0)
        path = synth.write_migan_gguf(tmp_path_factory.mktemp("migan_blocks") / "blocks.gguf", 16, sd=sd)
        _block_cache["sd"] = (migan_ref.f16_rounded(sd), path)
    return _block_cache["sd"]


@pytest.mark.parametrize("name,flags", [("plain", {}), ("down", dict(down=True)), ("upn", dict(up=True, noise=True)), ("noise", dict(noise=True))])
@pytest.mark.parametrize("fused", [True, False])
def test_separable_conv_against_reference(device, tmp_path_factory, name, flags, fused):
    sd, path = _block_weights(tmp_path_factory)
    x = R.f16(np.random.default_rng(5).standard_normal((NB, H0, W0, 16)))
    want = migan_ref.separable_conv(sd, name, x.astype(np.float32), **flags).astype(np.float64)
    g = G.Graph(device, G.Weights(path))
    g.set_fused_models(fused)
    m = G.ModelRef(g)
    xi = g.input((16, W0, H0, NB), G.F16, "x")
    y = g.output(G.migan_separable_conv_2d(m[name], xi, activation=True, downsample=flags.get("down", False), upsample=flags.get("up", False), noise=flags.get("noise", False)), "y")
    g.allocate()
    if fused:
        assert len(_lines(g)) == {"plain": 2, "down": 3, "upn": 3, "noise": 2}[name], _lines(g)
    g.set(xi, x)
    g.compute()
    _close(g.get(y), want, fused, f"separable_conv {name}")


@pytest.mark.parametrize("fused", [True, False])
def test_synthesis_block_against_reference(device, tmp_path_factory, fused):
    sd, path = _block_weights(tmp_path_factory)
    rng = np.random.default_rng(6)
    x = R.f16(rng.standard_normal((NB, H0, W0, 16)))
    feat = R.f16(rng.standard_normal((NB, 2 * H0, 2 * W0, 24)))
    img = np.zeros((NB, H0, W0, 8))
    img[..., :3] = R.f16(rng.standard_normal((NB, H0, W0, 3)) * 0.5)
    f32 = lambda a: a.astype(np.float32)
    wx = migan_ref.separable_conv(sd, "blk.conv1", f32(x), up=True, noise=True) + f32(feat)
    wx = migan_ref.separable_conv(sd, "blk.conv2", wx, noise=True)
    wimg = migan_ref.upsample(f32(img[..., :3]), sd["blk.upsample.filter.weight"], sd["blk.upsample.filter_const"]) + migan_ref.conv1x1(wx, sd["blk.torgb.weight"], sd["blk.torgb.bias"])
    g = G.Graph(device, G.Weights(path))
    g.set_fused_models(fused)
    m = G.ModelRef(g)
    xi, fi, ii = g.input((16, W0, H0, NB), G.F16, "x"), g.input((24, 2 * W0, 2 * H0, NB), G.F16, "feat"), g.input((8, W0, H0, NB), G.F16, "img")
    xo, io = G.migan_synthesis_block(m["blk"], xi, fi, ii, upsample=True, noise=True)
    g.output(xo, "xo")
    g.output(io, "io")
    g.allocate()
    if fused:
        assert [l.split("[")[0].split()[0] for l in _lines(g)] == ["dwconv3x3", "conv1x1", "upfirdn2x", "dwconv3x3", "gemm(conv1x1)", "conv1x1", "upfirdn2x"], _lines(g)
    for t, a in ((xi, x), (fi, feat), (ii, img)):
        g.set(t, a)
    g.compute()
    _close(g.get(xo), wx.astype(np.float64), fused, "synthesis_block x")
    got_img = g.get(io)
    assert (got_img[..., 3:] == 0).all(), "channels 3..7 of the image path are exact zeros"
    _close(got_img[..., :3], wimg.astype(np.float64), fused, "synthesis_block img")


# ---- groups that meet in one add, groups next to other lowerings' patterns (tests/test_graph_migan_cpu.py has their launch lists) ---------------------------

from test_graph_migan_cpu import MEETING, meeting_graphs  # noqa: E402


@pytest.mark.parametrize("which", MEETING)
def test_meeting_groups_fused_against_per_node(device, which):
    got = {}
    for fused in (True, False):
        g = G.Graph(device)
        g.set_fused_models(fused)
        ins, out = meeting_graphs(g, which)
        g.allocate()
        for i, t in enumerate(ins):
            g.set(t, R.f16(np.random.default_rng(90 + i).standard_normal(t.ne[::-1]) * 2))
        g.compute()
        got[fused] = g.get(out)
    _close(got[True], got[False].astype(np.float64), "both", which)


# ---- the generator --------------------------------------------------------------------------------------------------------------------------------------

def _inputs(n, res, seed):
    rng = np.random.default_rng(seed)
    imgs = synth.images(n, res, res, seed=seed)
    masks = np.zeros((n, res, res), np.uint8)
    for i in range(n):
        y0, x0 = rng.integers(0, res // 2, 2)
        masks[i, y0:y0 + res // 3, x0:x0 + res // 4] = 255
    return np.stack([migan_ref.preprocess(imgs[i], masks[i], res) for i in range(n)])


_gen_cache = {}


def _gen_case(tmp_path_factory, res, changed=False, **ch):
    key = (res, changed, tuple(sorted(ch.items())))
    if key not in _gen_cache:
        sd = synth.migan_state_dict(res, seed=3, **ch)
        if changed:  # one filter_const entry that is not the zero-insertion tile's: that group stays per node
            k = f"synthesis.b{res}.conv1.upsample.filter_const"
            sd[k] = sd[k].copy()
            sd[k][0, 0, 3, 5] = 1.0
        path = synth.write_migan_gguf(tmp_path_factory.mktemp("migan_gen") / f"gen{res}.gguf", res, sd=sd)
        x4 = _inputs(2, res, 40 + res)
        want = migan_ref.generate(migan_ref.f16_rounded(sd), x4, res).astype(np.float64)
        want.setflags(write=False)
        _gen_cache[key] = (path, x4, want)
    return _gen_cache[key]


def _run(device, path, x4, res, fused, hip_graph=False):
    g = G.Graph(device, G.Weights(path))
    g.set_fused_models(fused)
    xi = g.input((4, res, res, x4.shape[0]), G.F32, "image")
    out = G.migan_generate(G.ModelRef(g), xi, res)
    g.allocate()
    g.set(xi, x4)
    g.compute()
    first = g.get(out)
    if hip_graph:
        g.use_hip_graph(True)
        g.compute()  # records
        g.compute()  # replays
        np.testing.assert_array_equal(g.get(out), first)  # the hipGraph replay is bit-identical to the direct run
    return first, g


@pytest.mark.parametrize("res", [16, 32])
@pytest.mark.parametrize("fused", [True, False])
def test_generate_against_reference(device, tmp_path_factory, res, fused):
    path, x4, want = _gen_case(tmp_path_factory, res, **CH)
    got, g = _run(device, path, x4, res, fused, hip_graph=True)
    assert got.shape == (2, res, res, 3)
    _close(got, want, fused, f"migan_generate res {res}")
    alone, _ = _run(device, path, x4[:1], res, fused)
    np.testing.assert_array_equal(alone[0], got[0])  # image 0 alone gives the bits it gives in the batch


def test_generate_with_a_changed_filter_const_agrees_with_per_node(device, tmp_path_factory):
    path, x4, want = _gen_case(tmp_path_factory, 32, changed=True, **CH)
    fused, g = _run(device, path, x4, 32, True)
    lines = _lines(g)
    assert sum(l.startswith("upfirdn2x") for l in lines) == 5 and sum(l.startswith("nearest") for l in lines) == 1, lines
    per_node, _ = _run(device, path, x4, 32, False)
    _close(fused, want, False, "changed filter_const, fused")
    _close(per_node, want, False, "changed filter_const, per node")
    _close(fused, per_node.astype(np.float64), "both", "changed filter_const")


def test_generate_agrees_with_the_hand_schedule(device, tmp_path_factory):
    """widths that are multiples of 64 (all 64 here), which csrc/migan.cpp's schedule takes: the two paths agree, and both with the reference"""
    path, x4, want = _gen_case(tmp_path_factory, 32, ch_base=2048, ch_max=64)
    got, g = _run(device, path, x4, 32, True)
    hand = vision.Migan.load(path, device).generate(x4)
    _close(got, want, True, "graph, 64-wide")
    _close(hand, want, True, "hand schedule, 64-wide")
    _close(got, hand.astype(np.float64), True, "graph against hand schedule")

"""-m gpu: the graph executor's glue launchers (kernels_graph.hip) and the per-family pre / post-processing launchers, each called directly through
the vx_* C ABI and compared with a float64 restatement of its contract in include/visp_hip_kernels.h (tests/graph_ref.py). Data movement and
conversions are bit-exact; arithmetic is held to the bound its rounding steps allow, stated per test."""
import ctypes as C

import numpy as np
import pytest

import graph_ref as R
from visioncpp_amd import _lib as L

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _device():
    api = L.get_lib()
    assert api.vx_device_count() > 0, "no HIP device visible: the product path has no CPU fallback"
    L.vx_check(api.vx_set_device(0))
    yield


@pytest.fixture(autouse=True)
def _release_buffers():
    yield
    release()


from gpu_util import api, dev, empty, release, sync  # noqa: E402

F32_EPS = 2.0 ** -24  # unit roundoff of f32


def _i64(v):
    return (C.c_int64 * 4)(*[int(x) for x in v])


def _at(buf, byte_offset=0):
    return C.c_void_p(buf.ptr + byte_offset)


def _bits(a):
    return np.asarray(a, np.float16).view(np.uint16)


def _special_f16(rng, n):
    """Random f16 values mixed with the edges: +-0, subnormals, the largest normal, values near 1."""
    v = (rng.standard_normal(n) * 4).astype(np.float16)
    edge = np.array([0.0, -0.0, 6e-8, -6e-8, 2.0 ** -24, 3 * 2.0 ** -24, -(2.0 ** -15), 2.0 ** -14, 65504.0, -65504.0, 1.0, -1.0, 0.5, -3.0], np.float16)
    k = min(n, edge.size)
    v[:k] = edge[:k]
    return v


# ---- vx_unary_f16 ----------------------------------------------------------------------------------------------------------

UNARY_OPS = [(0, 0.0), (1, 0.0), (2, 1.5), (2, 4096.0), (3, 0.0), (3, 0.2), (3, 1.0), (3, 1.5), (3, -0.5)]


@pytest.mark.parametrize("n,op,s", [(n, op, s) for n in (1, 7, 8, 9, 1000003) for op, s in UNARY_OPS] +
                         [(2 ** 25 + 13, op, s) for op, s in ((0, 0.0), (1, 0.0), (2, 1.5), (3, 1.5))])
def test_unary_f16(n, op, s):
    """Ops 0-3 on the vector body, the n % 8 tail and, at 2^25 + 13 elements (past blocks_for's 16384-block cap), the grid-stride loop. scale 4096
    overflows to inf; leaky slopes outside [0, 1] tell ggml's x > 0 ? x : s x from max(x, s x)."""
    rng = np.random.default_rng(n + op)
    x = _special_f16(rng, n)
    xd, yd = dev(x), empty(n * 2 + 16)
    canary = np.full(8, 12345, np.uint16)
    L.vx_check(api().vx_memcpy_h2d(_at(yd, n * 2), canary.ctypes.data_as(C.c_void_p), 16, None))
    L.vx_check(api().vx_unary_f16(op, xd.ptr, yd.ptr, n, s, None))
    sync()
    got = yd.to_numpy(np.float16, (n + 8,))
    assert (got[n:].view(np.uint16) == 12345).all(), "wrote past n"
    got = got[:n]
    x64 = x.astype(np.float64)
    if op == 0:
        R.assert_f16_ulp(got, R.gelu(x64), R.GELU_F16_ULPS, "gelu")
    elif op == 1:
        np.testing.assert_array_equal(got.astype(np.float64), R.relu(x64))  # exact (values: max(-0, 0) may give either zero)
    elif op == 2:
        R.assert_f16_ulp(got, R.scale(x64, s), 1.0, "scale")
    else:
        want = R.leaky_relu(x64, s)
        R.assert_f16_ulp(got, want, 1.0, f"leaky_relu {s}")
        if s == 1.5:  # what the max(x, s x) form got wrong: positive inputs pass through unscaled
            pos = x64 > 0
            np.testing.assert_array_equal(got[pos], x[pos])


# ---- vx_binary_rows --------------------------------------------------------------------------------------------------------

def _typed(a, f32):
    return np.asarray(a, np.float32 if f32 else np.float16)


@pytest.mark.parametrize("types", [(a, b, y) for a in (0, 1) for b in (0, 1) for y in (0, 1)])
@pytest.mark.parametrize("op", [0, 1])
@pytest.mark.parametrize("n,period", [(24 * 40, 1), (24 * 40, 3), (24 * 40, 8), (24 * 40, 24), (24 * 40, 24 * 40), (3 * 1001, 3), (5 * 77, 5 * 77)])
def test_binary_rows(types, op, n, period):
    """y = a (op) b[i mod period] for every (a, b, y) f16 / f32 combination; within 1 ulp of the output type of the float64 result (the kernel
    computes in f32 and rounds once more to f16)."""
    a_f32, b_f32, y_f32 = types
    rng = np.random.default_rng(n + period + op)
    a = _typed(rng.standard_normal(n) * 3, a_f32)
    b = _typed(rng.standard_normal(period) * 2, b_f32)
    ad, bd = dev(a), dev(b)
    yd = empty(n * (4 if y_f32 else 2))
    L.vx_check(api().vx_binary_rows(op, ad.ptr, a_f32, bd.ptr, b_f32, period, yd.ptr, y_f32, n, None))
    sync()
    got = yd.to_numpy(np.float32 if y_f32 else np.float16, (n,))
    want = R.binary("add" if op == 0 else "mul", a, b, period)
    if y_f32:
        np.testing.assert_array_less(np.abs(got - want), 2 * F32_EPS * np.abs(want) + 1e-45)
    else:
        R.assert_f16_ulp(got, want, 1.0, "binary")


@pytest.mark.parametrize("op", [0, 1])
@pytest.mark.parametrize("b_f32", [0, 1])
@pytest.mark.parametrize("which", ["a", "y"])
def test_binary_rows_scalar_path_matches_vector_path(op, b_f32, which):
    """The f16 fast path (16-byte aligned a and y, n and period multiples of 8) and the generic kernel must give the same bits: moving a or y by
    one element forces the generic one on the same data."""
    rng = np.random.default_rng(7 + op)
    n, period = 8 * 1000, 40
    a = rng.standard_normal(n).astype(np.float16)
    b = _typed(rng.standard_normal(period), b_f32)
    ad, a_off = dev(a), dev(np.concatenate([np.zeros(1, np.float16), a]))
    bd = dev(b)
    y_vec, y_off = empty(n * 2), empty(n * 2 + 16)
    L.vx_check(api().vx_binary_rows(op, ad.ptr, 0, bd.ptr, b_f32, period, y_vec.ptr, 0, n, None))
    a_src = _at(a_off, 2) if which == "a" else ad.ptr
    y_dst = _at(y_off, 2) if which == "y" else y_off.ptr
    L.vx_check(api().vx_binary_rows(op, a_src, 0, bd.ptr, b_f32, period, y_dst, 0, n, None))
    sync()
    v = y_vec.to_numpy(np.float16, (n,))
    s = y_off.to_numpy(np.float16, (n + 8,))[1: n + 1] if which == "y" else y_off.to_numpy(np.float16, (n,))
    np.testing.assert_array_equal(_bits(v), _bits(s))
    R.assert_f16_ulp(v, R.binary("add" if op == 0 else "mul", a, b, period), 1.0, "binary8")


# ---- vx_copy_strided_f16 ---------------------------------------------------------------------------------------------------

def _copy_ref(src, dst, ne, ss, ds, scale):
    i = np.meshgrid(*[np.arange(n) for n in ne], indexing="ij")
    si = sum(i[d] * ss[d] for d in range(4)).reshape(-1)
    di = sum(i[d] * ds[d] for d in range(4)).reshape(-1)
    v = src[si]
    if scale != 1.0:
        v = (v.astype(np.float32) * np.float32(scale)).astype(np.float16)  # the kernel's f32 product, rounded to f16
    out = dst.copy()
    out[di] = v
    return out


def _run_copy(src, dst_elems, ne, ss, ds, scale=1.0, src_off=0, dst_off=0):
    canary = np.full(dst_elems + dst_off, -7.25, np.float16)
    sd, dd = dev(np.concatenate([np.zeros(src_off, np.float16), src])), dev(canary)
    L.vx_check(api().vx_copy_strided_f16(_at(sd, 2 * src_off), _at(dd, 2 * dst_off), _i64(ne), _i64(ss), _i64(ds), scale, None))
    sync()
    return dd.to_numpy(np.float16, (dst_elems + dst_off,))[dst_off:]


COPIES = {
    # name: (ne, src strides, dst strides, source elements, destination elements)
    "rows_with_gaps": ((16, 5, 3, 2), (1, 16, 80, 240), (1, 24, 24 * 6, 24 * 6 * 4), 480, 24 * 6 * 4 * 2),
    "broadcast_d1": ((16, 6, 3, 2), (1, 0, 16, 48), (1, 16, 96, 288), 96, 576),
    "broadcast_d2": ((16, 6, 3, 2), (1, 16, 0, 96), (1, 16, 96, 288), 192, 576),
    "broadcast_d3": ((16, 6, 3, 2), (1, 16, 96, 0), (1, 16, 96, 288), 288, 576),
    "transpose_4d": ((8, 6, 4, 3), (24, 1, 6, 192), (1, 8, 48, 192), 576, 576),
}


@pytest.mark.parametrize("name", sorted(COPIES))
@pytest.mark.parametrize("scale", [1.0, 0.2])
def test_copy_strided_vector_and_scalar_paths(name, scale):
    """One logical copy through the 8-wide kernel (16-byte aligned, strides multiples of 8) and through the generic one (the same copy one element
    into both buffers): bit-identical, equal to the reference, and every destination element outside the selection keeps its canary."""
    ne, ss, ds, n_src, n_dst = COPIES[name]
    rng = np.random.default_rng(len(name))
    src = rng.standard_normal(n_src).astype(np.float16)
    canary = np.full(n_dst, -7.25, np.float16)
    want = _copy_ref(src, canary, ne, ss, ds, scale)
    vec = _run_copy(src, n_dst, ne, ss, ds, scale)
    sca = _run_copy(src, n_dst, ne, ss, ds, scale, src_off=1, dst_off=1)
    np.testing.assert_array_equal(_bits(vec), _bits(want))
    np.testing.assert_array_equal(_bits(sca), _bits(want))
    if scale != 1.0:  # and within 1 f16 ulp of the float64 product
        ref64 = _copy_ref(src.astype(np.float64), np.full(n_dst, np.nan), ne, ss, ds, 1.0) * scale
        sel = ~np.isnan(ref64)
        R.assert_f16_ulp(vec[sel], ref64[sel], 1.0, "copy scale")


def test_copy_strided_odd_rows_take_the_generic_kernel():
    """Rows of 5 elements (no 8-wide path at all), a stride-3 source walk and a scale: the generic kernel against the reference."""
    rng = np.random.default_rng(11)
    src = rng.standard_normal(400).astype(np.float16)
    ne, ss, ds = (5, 7, 2, 3), (3, 17, 130, 1), (1, 6, 48, 100)
    got = _run_copy(src, 300, ne, ss, ds, -1.5)
    np.testing.assert_array_equal(_bits(got), _bits(_copy_ref(src, np.full(300, -7.25, np.float16), ne, ss, ds, -1.5)))


# ---- vx_nearest_f16 --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B,H,W,OH,OW", [(2, 5, 5, 9, 9), (1, 7, 7, 3, 3), (3, 19, 19, 37, 37), (2, 5, 7, 9, 21), (1, 8, 6, 16, 12), (2, 37, 19, 19, 37)])
@pytest.mark.parametrize("C", [8, 64])
def test_nearest(B, H, W, OH, OW, C):
    """ggml's nearest index floor(i / (float)(out / in)) at up, down and non-integer ratios; exact. Where torch's nearest picks the same source (it
    uses in / out instead), the two agree."""
    import torch
    import torch.nn.functional as F

    rng = np.random.default_rng(B * H * W + C)
    x = rng.standard_normal((B, H, W, C)).astype(np.float16)
    yd = empty(B * OH * OW * C * 2)
    L.vx_check(api().vx_nearest_f16(dev(x).ptr, yd.ptr, B, H, W, C, OH, OW, None))
    sync()
    got = yd.to_numpy(np.float16, (B, OH, OW, C))
    np.testing.assert_array_equal(_bits(got), _bits(R.interpolate_nearest(x, OW, OH)))
    tv = F.interpolate(torch.from_numpy(x.astype(np.float32)).permute(0, 3, 1, 2), size=(OH, OW), mode="nearest").permute(0, 2, 3, 1).numpy()
    ty = np.floor(np.arange(OH) * (H / OH)).astype(int)
    tx = np.floor(np.arange(OW) * (W / OW)).astype(int)
    agree = (ty == R.nearest_index(OH, H))[:, None] & (tx == R.nearest_index(OW, W))[None, :]
    np.testing.assert_array_equal(got.astype(np.float32)[:, agree], tv[:, agree])


# ---- vx_convert ------------------------------------------------------------------------------------------------------------

def test_convert_both_directions():
    """f32 -> f16 rounds to nearest even (ties, overflow to inf, subnormals, NaN); f16 -> f32 is exact."""
    one = 1.0
    special = np.array([0.0, -0.0, 1.0, one + 2.0 ** -11, one + 3 * 2.0 ** -11, -(one + 2.0 ** -11), 2.0 ** -25, 3 * 2.0 ** -25, 2.0 ** -24 * 1.5,
                        1e-7, -1e-7, 6.1e-5, 65504.0, 65519.0, 65520.0, 70000.0, -1e6, np.inf, -np.inf, np.nan, 1e-30], np.float32)
    rng = np.random.default_rng(2)
    x = np.concatenate([special, (rng.standard_normal(100003) * 100).astype(np.float32)])
    n = x.size
    yd = empty(n * 2)
    L.vx_check(api().vx_convert(dev(x).ptr, 1, yd.ptr, 0, n, None))
    sync()
    got = yd.to_numpy(np.float16, (n,))
    with np.errstate(over="ignore"):
        want = x.astype(np.float16)
    nan = np.isnan(want)
    assert np.isnan(got[nan]).all()
    np.testing.assert_array_equal(_bits(got[~nan]), _bits(want[~nan]))
    h = got
    zd = empty(n * 4)
    L.vx_check(api().vx_convert(dev(h).ptr, 0, zd.ptr, 1, n, None))
    sync()
    back = zd.to_numpy(np.float32, (n,))
    nan = np.isnan(h)
    assert np.isnan(back[nan]).all()
    np.testing.assert_array_equal(back[~nan].view(np.uint32), h[~nan].astype(np.float32).view(np.uint32))


# ---- vx_im2col_patches_f32 -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ps,C,H,W,extra", [(1, 3, 3, 5, 5), (14, 3, 28, 42, 6), (16, 4, 32, 48, 64), (14, 4, 14, 28, 0)])
def test_im2col_patches(ps, C, H, W, extra):
    """rows (b, py, px), k = (ky, kx, c), each value rounded to f16, zero in the padding columns up to Kp; exact."""
    B = 2
    kreal = ps * ps * C
    Kp = -(-(kreal + extra) // 8) * 8
    rng = np.random.default_rng(ps + C)
    x = rng.standard_normal((B, H, W, C)).astype(np.float32)
    ph, pw = H // ps, W // ps
    out = empty(B * ph * pw * Kp * 2, zero=False)
    L.vx_check(api().vx_memset(out.ptr, 0x7B, B * ph * pw * Kp * 2, None))  # not zero: the kernel must write the padding itself
    L.vx_check(api().vx_im2col_patches_f32(dev(x).ptr, out.ptr, B, H, W, C, ps, Kp, None))
    sync()
    got = out.to_numpy(np.float16, (B * ph * pw, Kp))
    want = np.zeros((B * ph * pw, Kp), np.float16)
    want[:, :kreal] = x.reshape(B, ph, ps, pw, ps, C).transpose(0, 1, 3, 2, 4, 5).reshape(B * ph * pw, kreal).astype(np.float16)
    np.testing.assert_array_equal(_bits(got), _bits(want))


# ---- vx_image_planes_f32 ---------------------------------------------------------------------------------------------------

IMAGE_RESIDUE_BOUND = 2.0 ** -24  # |hi + lo - x| for x in [0, 1]: the residue is below 2^-12, where f16's spacing is at most 2^-23


@pytest.mark.parametrize("C", [1, 3, 4, 16])
def test_image_planes(C):
    """32 f16 channels per pixel: hi = f16(x), lo = f16(x - hi), zeros from 2C on; exact. The reconstruction hi + lo is NOT x: on the u8 levels
    k / 255 and on random f32 in [0, 1] it stays within 2^-24, and the bound is reached."""
    rng = np.random.default_rng(C)
    levels = np.arange(256, dtype=np.float32) / np.float32(255.0)
    x = np.concatenate([np.resize(levels, 256 * C), rng.random(4099 * C, dtype=np.float32)]).astype(np.float32)
    n_pix = x.size // C
    x = x[: n_pix * C]
    yd = empty(n_pix * 64, zero=False)
    L.vx_check(api().vx_memset(yd.ptr, 0x55, n_pix * 64, None))
    L.vx_check(api().vx_image_planes_f32(dev(x).ptr, yd.ptr, n_pix, C, None))
    sync()
    got = yd.to_numpy(np.float16, (n_pix, 32))
    xx = x.reshape(n_pix, C)
    hi = xx.astype(np.float16)
    lo = (xx - hi.astype(np.float32)).astype(np.float16)
    np.testing.assert_array_equal(_bits(got[:, :C]), _bits(hi))
    np.testing.assert_array_equal(_bits(got[:, C: 2 * C]), _bits(lo))
    assert not got[:, 2 * C:].astype(np.float32).any()
    err = np.abs(got[:, :C].astype(np.float64) + got[:, C: 2 * C].astype(np.float64) - xx.astype(np.float64))
    assert err.max() <= IMAGE_RESIDUE_BOUND
    lvl = err.reshape(-1)[:256]  # the levels 0 / 255 .. 255 / 255, in order
    assert int((lvl != 0).sum()) == 159 and lvl.max() == IMAGE_RESIDUE_BOUND  # 159 of the 256 levels are not exact, and the bound is reached


# ---- vx_conv1x1_to1_f32 ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("C", [8, 32, 1024])
@pytest.mark.parametrize("relu,scale", [(0, 1.0), (1, 1.0), (1, 20.0), (0, -0.5)])
def test_conv1x1_to1(C, relu, scale):
    """out = scale * act(sum_c x w + bias) with an f32 fma chain over C: |error| <= (C + 2) u (sum |x w| + |bias|) |scale| + u |out| (u = 2^-24)."""
    M = 1000 + C % 7 + 3  # not a multiple of 256
    rng = np.random.default_rng(C + relu)
    x = rng.standard_normal((M, C)).astype(np.float16)
    w = (rng.standard_normal(C) / np.sqrt(C)).astype(np.float32)
    bias = 0.3
    od = empty(M * 4)
    L.vx_check(api().vx_conv1x1_to1_f32(dev(x).ptr, dev(w).ptr, bias, relu, scale, od.ptr, M, C, None))
    sync()
    got = od.to_numpy(np.float32, (M,)).astype(np.float64)
    acc = x.astype(np.float64) @ w.astype(np.float64) + np.float64(np.float32(bias))
    want = (np.maximum(acc, 0) if relu else acc) * scale
    bound = (C + 2) * F32_EPS * (np.abs(x.astype(np.float64)) @ np.abs(w.astype(np.float64)) + bias) * abs(scale) + F32_EPS * np.abs(want)
    assert (np.abs(got - want) <= bound).all()


# ---- family launchers ------------------------------------------------------------------------------------------------------

def _lrelu_agc(v):
    return np.clip(np.where(v < 0, 0.2 * v, v) * np.sqrt(2.0), -256.0, 256.0)


@pytest.mark.parametrize("mode", ["u8_3", "u8_4", "in4"])
def test_migan_preprocess(mode):
    """out f16 [n, C] = lrelu_agc(fromrgb(p)): p = {a - 0.5, a (2 v / 255 - 1)} with a = 1 - mask / 255 from the image and mask, or p = in4. f32
    arithmetic, then f16: within 1 f16 ulp plus the f32 error of p and of the 4-term fma chain (10 u of sum |p w| + |b| + |t|, times sqrt2)."""
    rng = np.random.default_rng(len(mode))
    n, Cc = 777, 32
    w = (rng.standard_normal((Cc, 4)) * 2).astype(np.float32)
    b = rng.standard_normal(Cc).astype(np.float32) * 0.5
    od = empty(n * Cc * 2)
    if mode == "in4":
        p = (rng.standard_normal((n, 4)) * 60).astype(np.float32)  # large enough to reach the +-256 clamp
        L.vx_check(api().vx_migan_preprocess(None, 0, None, dev(p).ptr, dev(w).ptr, dev(b).ptr, od.ptr, n, Cc, None))
        p64 = p.astype(np.float64)
    else:
        ch = 3 if mode == "u8_3" else 4
        img = rng.integers(0, 256, (n, ch), dtype=np.uint8)
        mask = rng.integers(0, 256, n, dtype=np.uint8)
        mask[:4] = [0, 255, 128, 1]
        L.vx_check(api().vx_migan_preprocess(dev(img).ptr, ch, dev(mask).ptr, None, dev(w).ptr, dev(b).ptr, od.ptr, n, Cc, None))
        a = 1.0 - mask.astype(np.float64) / 255.0
        p64 = np.concatenate([(a - 0.5)[:, None], a[:, None] * (img[:, :3].astype(np.float64) / 255.0 * 2.0 - 1.0)], 1)
    sync()
    got = od.to_numpy(np.float16, (n, Cc)).astype(np.float64)
    t = p64 @ w.T.astype(np.float64) + b
    want = _lrelu_agc(t)
    slack = 10 * F32_EPS * (np.abs(p64) @ np.abs(w.T.astype(np.float64)) + np.abs(b) + np.abs(t)) * np.sqrt(2.0)
    assert (np.abs(got - R.f16(want)) <= R.f16_ulp(want) + slack).all()
    if mode == "in4":
        assert (np.abs(got) == 256).any()


def test_migan_postprocess():
    """rgba = trunc(clamp(v * 0.5 + 0.5, 0, 1) * 255) with each step rounded to f32, alpha = mask: exact, at the clamp limits and where x 255 lands
    just below / above an integer (truncation, not rounding)."""
    rng = np.random.default_rng(4)
    k = np.arange(256, dtype=np.float32)
    t = np.concatenate([k / 255, np.nextafter(k / 255, np.float32(-1)), np.nextafter(k / 255, np.float32(2)), (k + np.float32(0.9)) / 255]).astype(np.float32)
    v = np.concatenate([(t - np.float32(0.5)) * np.float32(2), np.array([-1, 1, -1.5, 1.5, -100, 100, 0, -0.0, np.inf, -np.inf], np.float32),
                        rng.uniform(-1.2, 1.2, 3000).astype(np.float32)])
    v = np.resize(v, (v.size + 2) // 3 * 3).astype(np.float32)
    n = v.size // 3
    mask = rng.integers(0, 256, n, dtype=np.uint8)
    od = empty(n * 4)
    L.vx_check(api().vx_migan_postprocess(dev(v).ptr, dev(mask).ptr, od.ptr, n, None))
    sync()
    got = od.to_numpy(np.uint8, (n, 4))
    tt = (v * np.float32(0.5)).astype(np.float32) + np.float32(0.5)
    want = (np.clip(tt, 0, 1).astype(np.float32) * np.float32(255)).astype(np.float32)
    np.testing.assert_array_equal(got[:, :3].reshape(-1), np.trunc(want).astype(np.uint8))
    np.testing.assert_array_equal(got[:, 3], mask)
    assert (np.trunc(want) != np.round(want)).any()  # the data do tell truncation from rounding


@pytest.mark.parametrize("src", ["rgb", "rgba", "f32"])
def test_yolo_preprocess(src):
    """f16 [n][8] = v / 255 (u8, alpha ignored) or v (f32 rgb), channels 3..7 zero; exact (f32 quotient, then f16)."""
    rng = np.random.default_rng(len(src))
    n = 1237
    od = empty(n * 16, zero=False)
    L.vx_check(api().vx_memset(od.ptr, 0x3C, n * 16, None))
    if src == "f32":
        x = (rng.standard_normal((n, 3)) * 2).astype(np.float32)
        L.vx_check(api().vx_yolo_preprocess(None, 3, dev(x).ptr, od.ptr, n, None))
        want = x.astype(np.float16)
    else:
        ch = 3 if src == "rgb" else 4
        img = rng.integers(0, 256, (n, ch), dtype=np.uint8)
        img[:256, 0] = np.arange(256)
        L.vx_check(api().vx_yolo_preprocess(dev(img).ptr, ch, None, od.ptr, n, None))
        want = (img[:, :3].astype(np.float32) / np.float32(255)).astype(np.float16)
    sync()
    got = od.to_numpy(np.float16, (n, 8))
    np.testing.assert_array_equal(_bits(got[:, :3]), _bits(want))
    assert not got[:, 3:].astype(np.float32).any()


def _tiles_ref(img, layout, order):
    """Every tile pixel = the image pixel at the tile's source position (clamped to the image), channels picked by `order`, in [tiles, h, w, 3]."""
    B, h, w, _ = img.shape
    iw, ih, ox, oy, nx, ny, tw, th = layout
    out = np.empty((B, ny, nx, th, tw, 3), np.uint8)
    for cy in range(ny):
        for cx in range(nx):
            sy = np.minimum(cy * (th - oy) + np.arange(th), h - 1)
            sx = np.minimum(cx * (tw - ox) + np.arange(tw), w - 1)
            out[:, cy, cx] = img[:, sy][:, :, sx][..., list(order)]
    return out.reshape(B * ny * nx, th, tw, 3)


@pytest.mark.parametrize("fmt,ch,order", [(0, 4, (0, 1, 2)), (3, 3, (0, 1, 2)), (1, 4, (2, 1, 0))])
def test_esrgan_tiles_in(fmt, ch, order):
    """An overlapping tile layout that does not divide the image: the f32 tiles hold v / 255 at each tile's source position (exact), and the f16
    value | residue tiles of vx_esrgan_tiles_in reconstruct that value within the image-plane bound."""
    rng = np.random.default_rng(fmt)
    B, h, w = 2, 29, 37
    layout = (w, h, 4, 3, 3, 3, 16, 12)  # 3 x 3 tiles of 16 x 12, overlaps 4 / 3: 40 x 30 covers the 37 x 29 image
    img = rng.integers(0, 256, (B, h, w, ch), dtype=np.uint8)
    t = L.TileLayout(*layout)
    n_px = B * 9 * 16 * 12
    of, oh = empty(n_px * 12), empty(n_px * 64)
    idev = dev(img)
    L.vx_check(api().vx_esrgan_tiles_in_f32(idev.ptr, B, w, h, fmt, C.byref(t), of.ptr, None))
    L.vx_check(api().vx_esrgan_tiles_in(idev.ptr, B, w, h, fmt, C.byref(t), oh.ptr, None))
    sync()
    want = _tiles_ref(img, layout, order).astype(np.float32) / np.float32(255)
    got = of.to_numpy(np.float32, want.shape)
    np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))
    planes = oh.to_numpy(np.float16, (B * 9, 12, 16, 32)).astype(np.float64)
    recon = planes[..., :3] + planes[..., 3:6]
    assert np.abs(recon - want.astype(np.float64)).max() <= IMAGE_RESIDUE_BOUND
    assert not planes[..., 6:].any()


@pytest.mark.parametrize("C,ldy", [(96, 104), (256, 264), (520, 528)])
@pytest.mark.parametrize("out_f32", [0, 1])
def test_swin_layernorm_strided(C, ldy, out_f32):
    """Plain LayerNorm rows written with a row stride ldy > C: the gap columns keep their canary. f32 statistics over C terms: |error| <= 4 C u (|w x^| + |b|)
    + 1 ulp of the output type."""
    rng = np.random.default_rng(C + out_f32)
    rows = 333
    x = (rng.standard_normal((rows, C)) * 2 + 0.5).astype(np.float16)
    w = (1 + 0.2 * rng.standard_normal(C)).astype(np.float32)
    b = (0.1 * rng.standard_normal(C)).astype(np.float32)
    canary = np.full((rows, ldy), -3.0, np.float32 if out_f32 else np.float16)
    yd = dev(canary)
    L.vx_check(api().vx_swin_layernorm_strided_f16(dev(x).ptr, dev(w).ptr, dev(b).ptr, yd.ptr, rows, C, 1e-5, ldy, out_f32, None))
    sync()
    got = yd.to_numpy(np.float32 if out_f32 else np.float16, (rows, ldy))
    assert (got[:, C:] == -3.0).all(), "the gap columns were written"
    want = R.layer_norm(x.astype(np.float64), w, b, 1e-5)
    xhat = np.abs((want - b) / w)
    slack = C * F32_EPS * (np.abs(w) * xhat + np.abs(b)) * 4
    err = np.abs(got[:, :C].astype(np.float64) - (want if out_f32 else R.f16(want)))
    out_ulp = F32_EPS * 2 * np.abs(want) if out_f32 else R.f16_ulp(want)
    assert (err <= out_ulp + slack).all(), float((err - out_ulp - slack).max())

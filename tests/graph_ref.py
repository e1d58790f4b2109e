"""Float64 reference of the graph executor's generic ops, in ggml's conventions (a helper module of the tests, not a fixture).

Arrays are numpy arrays in numpy index order, i.e. the reversed ggml ne: a tensor of ne [C, W, H, B] is an array of shape (B, H, W, C), so ne[0]
is the last (contiguous) axis. Every function computes in float64; `f16` rounds where the executor holds a value in f16. The tolerances the tests
state follow from that arithmetic: data movement and relu are exact, one f16 rounding of the float64 result is the bound of scale / leaky_relu /
add / mul, and gelu stays within one f16 ulp although the kernels use the exp2 / rcp approximations (`GELU_F16_ULPS`)."""
from __future__ import annotations

import numpy as np

F16_MAX = 65504.0
# tanh-GELU of kernels_graph.hip: x * rcp(1 + exp2(x * w(x))) on f32 with the hardware exp2 / rcp (about 1 f32 ulp each), then rounded to f16. The
# f32 expression is a chain of products with no cancellation: its relative error is a few f32 ulps plus ln2 times the rounding of the exp2 argument
# x w, which only matters where exp2 is neither 0 nor huge (|x| <= 4: below 2e-6). That is far below half an f16 ulp (2^-12 relative), so the f16
# result is the correctly rounded one or its neighbour: within 1 f16 ulp of the float64 gelu rounded to f16.
GELU_F16_ULPS = 1.0


def f16(a) -> np.ndarray:
    """Round to f16 and back: what an f16 buffer of the executor holds (overflow to +-inf, ties to even)."""
    with np.errstate(over="ignore"):
        return np.asarray(a, np.float64).astype(np.float16).astype(np.float64)


def f16_ulp(a) -> np.ndarray:
    """The spacing of f16 at |a| (2^-24 in the subnormal range)."""
    a = np.abs(np.asarray(a, np.float64))
    e = np.floor(np.log2(np.maximum(a, 2.0 ** -14)))
    return 2.0 ** (e - 10)


def within_f16_ulp(got, want64, ulps=1.0) -> np.ndarray:
    """Elementwise: got is within `ulps` f16 ulps of the float64 result rounded to f16 (equal infinities and NaNs pass)."""
    got = np.asarray(got, np.float64)
    want = f16(want64)
    both_nan = np.isnan(got) & np.isnan(want)
    with np.errstate(invalid="ignore"):
        same_inf = np.isinf(want) & (got == want)
        close = np.abs(got - want) <= ulps * f16_ulp(want)
    return both_nan | same_inf | close


def assert_f16_ulp(got, want64, ulps=1.0, what=""):
    ok = within_f16_ulp(got, want64, ulps)
    if not ok.all():
        idx = np.argwhere(~ok)[:5]
        g, w = np.asarray(got, np.float64), np.asarray(want64, np.float64)
        raise AssertionError(f"{what}: {int((~ok).sum())} of {ok.size} values off by more than {ulps} f16 ulp; e.g. at {idx.tolist()}: "
                             f"got {[g[tuple(i)] for i in idx]} want {[w[tuple(i)] for i in idx]}")


def conv3x3(x, w, b=None):
    """x (B, H, W, Cin), w OHWI (Cout, 3, 3, Cin), stride 1, zero padding 1 -> float64 (B, H, W, Cout)"""
    x, w = np.asarray(x, np.float64), np.asarray(w, np.float64)
    B, H, W, _ = x.shape
    xp = np.pad(x, ((0, 0), (1, 1), (1, 1), (0, 0)))
    out = np.zeros((B, H, W, w.shape[0]))
    for ky in range(3):
        for kx in range(3):
            out += xp[:, ky:ky + H, kx:kx + W] @ w[:, ky, kx].T
    return out if b is None else out + np.asarray(b, np.float64)


# ---- element-wise ------------------------------------------------------------------------------------------------------------

def broadcast_period(a_shape, b_shape) -> int:
    """graph.cpp broadcast_period in numpy order: b equals a in its leading ggml dimensions (trailing numpy axes) and is 1 in the rest."""
    a_ne, b_ne = tuple(a_shape)[::-1], tuple(b_shape)[::-1]
    a_ne, b_ne = a_ne + (1,) * (4 - len(a_ne)), b_ne + (1,) * (4 - len(b_ne))
    period, ones = 1, False
    for i in range(4):
        if not ones and b_ne[i] == a_ne[i]:
            period *= b_ne[i]
            continue
        if b_ne[i] == 1:
            ones = ones or a_ne[i] != 1
            continue
        raise ValueError(f"cannot broadcast {b_shape} onto {a_shape}")
    return period


def binary(op: str, a, b, period: int | None = None) -> np.ndarray:
    """y[i] = a[i] (op) b[i mod period] over the flat arrays, float64; the result has a's shape."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64).reshape(-1)
    period = b.size if period is None else period
    bb = np.resize(b[:period], a.size).reshape(a.shape)
    return a + bb if op == "add" else a * bb


def add(a, b):
    return binary("add", a, b, broadcast_period(np.shape(a), np.shape(b)))


def mul(a, b):
    return binary("mul", a, b, broadcast_period(np.shape(a), np.shape(b)))


def relu(x):
    return np.maximum(np.asarray(x, np.float64), 0.0)


def leaky_relu(x, slope):
    """ggml_leaky_relu: x > 0 ? x : slope * x (not max(x, slope x), which differs for slope > 1)."""
    x = np.asarray(x, np.float64)
    return np.where(x > 0, x, slope * x)


def scale(x, s):
    return np.asarray(x, np.float64) * s


def gelu(x):
    """ggml_gelu, the tanh form, in float64."""
    x = np.asarray(x, np.float64)
    return 0.5 * x * (1.0 + np.tanh(np.sqrt(2.0 / np.pi) * (x + 0.044715 * x ** 3)))


def layer_norm(x, w, b, eps):
    x = np.asarray(x, np.float64)
    mu = x.mean(-1, keepdims=True)
    var = ((x - mu) ** 2).mean(-1, keepdims=True)
    return (x - mu) / np.sqrt(var + eps) * np.asarray(w, np.float64) + np.asarray(b, np.float64)


# ---- data movement -----------------------------------------------------------------------------------------------------------

def slice_(x, *sel):
    """ml.cpp:746-768: per ggml dimension (begin, end, step) with Python-style negative begin / end, end clamped to the extent."""
    x = np.asarray(x)
    nd = x.ndim
    idx = [slice(None)] * nd
    for d, s in enumerate(sel):
        if s is None:
            continue
        if isinstance(s, int):
            s = (s, s + 1, 1)
        b, e, st = tuple(s) + (1,) * (3 - len(s))
        ext = x.shape[nd - 1 - d]
        b = b + ext if b < 0 else b
        e = e + ext if e < 0 else e
        e = min(e, ext)
        assert 0 <= b < e, "empty or out-of-range selection"
        idx[nd - 1 - d] = slice(b, e, max(st, 1))
    return x[tuple(idx)]


def concat(a, b, dim: int):
    """Concatenation along ggml dimension `dim` of 4-D arrays."""
    return np.concatenate([np.asarray(a), np.asarray(b)], axis=3 - dim)


def repeat(x, *ne):
    """ggml_repeat to ne (ggml order), each source dimension 1 or already equal."""
    x = np.asarray(x)
    x = x.reshape((1,) * (4 - x.ndim) + x.shape)
    target = tuple(ne)[::-1]
    return np.broadcast_to(x, target).copy()


def nearest_index(out: int, src: int) -> np.ndarray:
    """ggml upscale (NEAREST): source index floor(i / (float)(out / src)), the ratio and the quotient in float32 as ggml computes them."""
    sf = np.float32(out) / np.float32(src)
    i = np.arange(out, dtype=np.float32)
    return np.minimum(np.floor(i / sf).astype(np.int64), src - 1)


def interpolate_nearest(x, ow: int, oh: int):
    """x (B, H, W, C) -> (B, oh, ow, C)."""
    x = np.asarray(x)
    iy, ix = nearest_index(oh, x.shape[1]), nearest_index(ow, x.shape[2])
    return x[:, iy][:, :, ix]


# ---- images ------------------------------------------------------------------------------------------------------------------

def image_u8_to_f32(img, mean, inv_std):
    """(v / 255 - mean) * inv_std per channel, each step rounded to f32 the way the kernel evaluates it."""
    v = np.asarray(img, np.float32) / np.float32(255.0)
    return (v + (-np.asarray(mean, np.float32))) * np.asarray(inv_std, np.float32)


def image_normalize(x):
    """Per image: (x - min) / (max - min), a span below 1e-5 taken as 1 (image.cpp:565-575), with the kernel's f32 steps (x * (1 / d)) + (-min / d)."""
    x = np.asarray(x, np.float32)
    out = np.empty_like(x)
    for b in range(x.shape[0]):
        mn, mx = np.float32(x[b].min()), np.float32(x[b].max())
        d = np.float32(mx - mn)
        d = np.float32(1.0) if d < np.float32(1e-5) else d
        s = np.float32(1.0) / d
        out[b] = (x[b] * s).astype(np.float32) + np.float32(-mn * s)
    return out

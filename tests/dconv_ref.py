"""float64 reference of vx_dconv3x3_f16 and a derived per-element error allowance. Plain numpy, nothing from the device side.

`args` is a dict keyed by the fields of vx_dconv_args (include/visp_hip_kernels.h). A pointer is replaced by a FLAT numpy array that holds the
WHOLE buffer behind it plus `<name>_off`, the element the pointer points at (a slice of a wider NHWC map, a later plane of a planar buffer):
  x     f16 flat, x_off      element of (image b, source pixel p, channel 32 k + j) = x_off + b * pixels * xp + k * x_plane + p * xp + j, xp = x_pix or 32
                             (planar: x_pix = 0, x_plane = a whole plane; NHWC: x_pix = row width, x_plane = 32). The kernel reads through a buffer
                             descriptor that ends with the image (NHWC) resp. with the image's copy in the last plane (planar): what lies past it
                             reads as ZERO, whatever the memory holds -- a Cin padded 48 -> 64 relies on it for its last pixel.
  w     f16 flat             [cin/32][9 taps][cout][32], the four 16-byte groups of every (tap, n) row at position g ^ ((n >> 2) & 3)
  bias  f32 [cout] or None   head_w f32 [32]
  res1, res2  f16 flat, *_off, *_plane, *_pix  addressed like the output
  out_size, out_off          elements of the whole output buffer (f16, or f32 for the RGB / HEAD epilogues) and where `out` points
  stamps                     ignored (diagnostics)
`evaluate` returns three dicts keyed "out": the expected content of the whole buffer as the call leaves a zero-initialised one, the allowance of
every element, and which elements the call writes. An element the call must not write (other planes, the slack between cout and out_pix, the
guard behind the last image) has allowance 0, so one comparison `|got - want| <= allowance` also catches any stray store.

The contract (header): v = conv(x) + bias; act (1: max(v, 0.2 v), 2: relu); res1: v = v * s1 + res1; res2: v = v * s2 + res2 -- in that order, a
scale only together with its residual; x_residual: v = v * s1 + x[channels 0..63] in res1's place. up2: x is the half-size map, nearest. a_relu:
conv of relu(x). bil_hs / bil_ws: x is the small map, the conv runs on its bilinear align_corners resize with source coordinate
o / ((n_out - 1) / (n_src - 1)) (ggml's form). RGB: f32 [B, H, W, 3] = v[0:3]. HEAD: f32 [B, H, W] = head_scale * relu(sum_n relu(v)[n] head_w[n] +
head_bias).

The allowance (u16 = 2^-11, u32 = 2^-24), derived from the arithmetic and never from device output:
  accumulation  (K + 8) u32 (|x| (*) |w| + |bias|), K = 9 cin: an f32 sum of K exact f16 x f16 products in ANY order lies within (K - 1) u32 times the
                sum of magnitudes of the exact sum, whatever the MFMA's order and the chunk order; the 8 spare units pay for the bias, the
                0.2f of LeakyReLU and the one f32 multiplication of the identity fold. ReLU and LeakyReLU have Lipschitz constant 1.
  f16 roundings max(u16 |v|, 2^-25) per rounding on the way out: the staged tile, and one per residual step (a unit-scale step is one correctly
                rounded f16 add; a scaled one is f16(f32(v) * s + f32(r)), whose two f32 operations add 2 u32 (|v s| + |r|)).
  scales        everything carried into a residual step is multiplied by |s1| resp. |s2|.
  RGB, HEAD     no f16 rounding (the accumulators are stored resp. reduced as f32). HEAD: the accumulation terms weighted by |head_w|, a
                (32 + 8) u32 term on sum_n |relu(v)[n] head_w[n]| + |head_bias| for its own 32-term f32 dot product, all times |head_scale|.
  x_residual    the kernel adds x * i with i = f16(1 / s1) to the accumulators (K grows by 32, the magnitudes by |x i|) and multiplies by s1:
                it computes conv * s1 + x * (i s1), so |x| |i s1 - 1| is added (s1 as the f32 the call passes). Zero where the reciprocal is exact (0.2, -0.5, 1).
  bilinear      an input value is lerp2(lerp2(a, b, fx), lerp2(c, d, fx), fy) on packed f16, lerp2(v, w, f) = fma(f, w, fma(-f, v, v)): two
                roundings per lerp2, and a value passes two lerp2 in a row: 4 roundings of magnitudes <= M = max(|a|, |b|, |c|, |d|) (all
                intermediate values are convex combinations up to those roundings). Each weight is rounded to f16 (<= 2^-12 absolute) and
                multiplies a difference <= 2 M: 2 more units. The coordinate is computed in f32 (sf and the division: <= 3 u32 n_src absolute on
                f, times 2 M per axis). Per input value: (6 u16 + 12 u32 max(hs, ws)) M + 4 * 2^-25, pushed through |w| like the inputs."""
from __future__ import annotations

import numpy as np

U16, U32, TINY16 = 2.0 ** -11, 2.0 ** -24, 2.0 ** -25
DC_F16, DC_RGB_F32, DC_HEAD_F32 = 0, 1, 2
BIL_ROUNDINGS = 6


def _get(args, key, default=0):
    v = args.get(key)
    return default if v is None else v


def round16(x):
    """the allowance of one rounding of x to f16"""
    return np.maximum(U16 * np.abs(x), TINY16)


def accumulation_term(K: int, mag):
    """an f32 sum of K exact f16 x f16 products in any order, plus the 8 spare units (bias, ...): on the sum of magnitudes `mag`"""
    return (K + 8) * U32 * mag


def bilinear_term(big, n_src: int, value_roundings: int = BIL_ROUNDINGS - 2):
    """the interpolated input value's error: `value_roundings` f16 roundings of magnitudes <= big (4 with two fused lerp2 in a row), 2 units
    for the two weights rounded to f16, the f32 coordinate"""
    return ((value_roundings + 2) * U16 + 12 * U32 * n_src) * big + value_roundings * TINY16


def head_epilogue(z, e, mag, K, hw, hb, hs, exact_clip=False):
    """HEAD: hs * relu(sum_n relu(z)[n] hw[n] + hb) from conv sums z with input-error term e and magnitudes mag -> (want, allowance).
    exact_clip: a ReLU whose argument is below zero by more than its own error bound gives exactly 0 on the device too -- such a channel
    carries no error into the dot product, and such an output has allowance 0 (with it off, ReLU only has Lipschitz constant 1)."""
    t = np.maximum(z, 0.0)
    ez = e + accumulation_term(K, mag)
    if exact_clip:
        ez = np.where(z + ez < 0, 0.0, ez)
    dot = t @ hw + hb
    err = ez @ np.abs(hw) + (32 + 8) * U32 * (np.abs(t) @ np.abs(hw) + abs(hb))
    allow = err * abs(hs) + U32 * np.abs(dot * hs)
    if exact_clip:
        allow = np.where(dot + err < 0, 0.0, allow)
    return np.maximum(dot, 0.0) * hs, allow


def pack_w(w: np.ndarray, cin_pad: int | None = None, cout_pad: int | None = None) -> np.ndarray:
    """[cout, cin, 3, 3] -> the flat f16 weight buffer of the header (zero padded to cin_pad / cout_pad, multiples of 32)"""
    co, ci = w.shape[:2]
    cip, cop = cin_pad or -(-ci // 32) * 32, cout_pad or -(-co // 32) * 32
    wp = np.zeros((cop, cip, 3, 3), np.float16)
    wp[:co, :ci] = w.astype(np.float16)
    t = wp.reshape(cop, cip // 32, 4, 8, 9).transpose(1, 4, 0, 2, 3)  # [chunk][tap][n][group][8]
    out = np.empty_like(t)
    n = np.arange(cop)
    for g in range(4):
        out[:, :, n, g ^ ((n >> 2) & 3)] = t[:, :, n, g]
    return np.ascontiguousarray(out).reshape(-1)


def unpack_w(flat: np.ndarray, cin: int, cout: int) -> np.ndarray:
    """the flat weight buffer -> float64 [9 taps][cin][cout]"""
    t = np.asarray(flat).reshape(cin // 32, 9, cout, 4, 8)
    out = np.empty_like(t)
    n = np.arange(cout)
    for g in range(4):
        out[:, :, n, g] = t[:, :, n, g ^ ((n >> 2) & 3)]
    return out.reshape(cin // 32, 9, cout, 32).transpose(1, 0, 3, 2).reshape(9, cin, cout).astype(np.float64)


def source_extent(args):
    if _get(args, "bil_hs") > 0:
        return args["bil_hs"], args["bil_ws"]
    up = 1 if _get(args, "up2") else 0
    return args["H"] >> up, args["W"] >> up


def source_map(args) -> np.ndarray:
    """float64 [B, Hs, Ws, cin]: what the kernel's loads return for every source pixel and channel (zero past the buffer descriptor)"""
    B, cin = args["B"], args["cin"]
    Hs, Ws = source_extent(args)
    xp = _get(args, "x_pix") or 32
    plane = _get(args, "x_plane")
    nch = cin // 32
    span = Hs * Ws * xp if xp > 32 else (nch - 1) * plane + Hs * Ws * 32
    c = np.arange(cin)
    off = (c // 32 * plane + c % 32)[None, :] + (np.arange(Hs * Ws) * xp)[:, None]  # [pixel, channel] inside the image's descriptor
    inside = off < span
    x = np.asarray(args["x"])
    absolute = _get(args, "x_off") + (np.arange(B) * Hs * Ws * xp)[:, None, None] + off[None]
    vals = x[np.minimum(absolute, x.size - 1)].astype(np.float64)
    assert (absolute[:, inside] < x.size).all(), "the call reads past the input buffer"
    return np.where(inside[None], vals, 0.0).reshape(B, Hs, Ws, cin)


def bilinear_table(n_out: int, n_src: int, dtype=np.float64):
    """first source index and weight of the second one for every output row (column): coordinate o / sf, sf = (n_out - 1) / (n_src - 1)"""
    sf = dtype(n_out - 1) / dtype(n_src - 1) if n_out > 1 and n_src > 1 else dtype(n_out) / dtype(n_src)
    sc = np.arange(n_out).astype(dtype) / sf
    i0 = np.clip(np.floor(sc).astype(np.int64), 0, n_src - 1)
    f = np.clip(sc - i0.astype(dtype), dtype(0), dtype(1))
    return i0, np.minimum(i0 + 1, n_src - 1), f


def input_map(args):
    """-> (xin, dx): float64 [B, H, W, cin] the map the conv runs on, and the bound of the device's error on each of its values (zero unless
    the loader interpolates)"""
    src = source_map(args)
    H, W = args["H"], args["W"]
    if _get(args, "bil_hs") > 0:
        hs, ws = args["bil_hs"], args["bil_ws"]
        y0, y1, fy = bilinear_table(H, hs)
        x0, x1, fx = bilinear_table(W, ws)
        fy, fx = fy[None, :, None, None], fx[None, None, :, None]
        a, b, c, d = src[:, y0][:, :, x0], src[:, y0][:, :, x1], src[:, y1][:, :, x0], src[:, y1][:, :, x1]
        xin = (a * (1 - fx) + b * fx) * (1 - fy) + (c * (1 - fx) + d * fx) * fy
        big = np.maximum(np.maximum(np.abs(a), np.abs(b)), np.maximum(np.abs(c), np.abs(d)))
        dx = bilinear_term(big, max(hs, ws))
    else:
        up = 1 if _get(args, "up2") else 0
        xin = src[:, np.arange(H) >> up][:, :, np.arange(W) >> up]
        dx = np.zeros_like(xin)
    if _get(args, "a_relu"):
        xin = np.maximum(xin, 0.0)
    return xin, dx


def conv3x3(x: np.ndarray, w9: np.ndarray) -> np.ndarray:
    """x [B, H, W, cin], w9 [9][cin][cout] -> [B, H, W, cout], zero padding 1"""
    B, H, W, _ = x.shape
    xp = np.pad(x, ((0, 0), (1, 1), (1, 1), (0, 0)))
    out = np.zeros((B, H, W, w9.shape[2]))
    for tap in range(9):
        ky, kx = divmod(tap, 3)
        out += xp[:, ky:ky + H, kx:kx + W] @ w9[tap]
    return out


def out_index(args, which="out"):
    """flat element index of (b, y, x, n) in an f16 map addressed by <which>_off / _plane / _pix -> int64 [B, H, W, cout]"""
    B, H, W, cout = args["B"], args["H"], args["W"], args["cout"]
    pix = _get(args, which + "_pix") or 32
    n = np.arange(cout)
    p = np.arange(B * H * W).reshape(B, H, W, 1)
    return _get(args, which + "_off") + p * pix + (n // 32 * _get(args, which + "_plane") + n % 32)


def activation(z, act):
    return np.maximum(z, 0.2 * z) if act == 1 else (np.maximum(z, 0.0) if act == 2 else z)


def evaluate(args):
    """-> (want, allow, written): three dicts "out" -> flat array of the whole output buffer (float64, float64, bool)"""
    B, H, W, cin, cout, epi = args["B"], args["H"], args["W"], args["cin"], args["cout"], _get(args, "epi")
    w9 = unpack_w(args["w"], cin, cout)
    bias = np.asarray(args["bias"], np.float64) if args.get("bias") is not None else np.zeros(cout)
    xin, dx = input_map(args)
    z = conv3x3(xin, w9) + bias
    mag = conv3x3(np.abs(xin), np.abs(w9)) + np.abs(bias)
    e = conv3x3(dx, np.abs(w9)) if dx.any() else 0.0
    K = 9 * cin
    size = args["out_size"]
    want, allow, written = np.zeros(size), np.zeros(size), np.zeros(size, bool)
    p = np.arange(B * H * W).reshape(B, H, W)

    if epi == DC_RGB_F32:
        idx = p[..., None] * 3 + np.arange(3)
        want[idx], allow[idx], written[idx] = z[..., :3], (e + accumulation_term(K, mag))[..., :3], True
    elif epi == DC_HEAD_F32:
        hw = np.asarray(args["head_w"], np.float64)
        hb, hs = float(_get(args, "head_bias", 0.0)), float(_get(args, "head_scale", 0.0))
        want[p], allow[p] = head_epilogue(z, e, mag, K, hw, hb, hs)
        written[p] = True
    else:
        assert epi == DC_F16
        s1, s2 = float(_get(args, "s1", 1.0)), float(_get(args, "s2", 1.0))
        v = activation(z, _get(args, "act"))
        e = e + accumulation_term(K, mag)
        if _get(args, "x_residual"):
            assert cout == 64 and args.get("res1") is None
            x64 = input_map(dict(args, a_relu=0))[0][..., :64]  # the header's x, not relu(x)
            inv = float(np.float16(np.float32(1.0) / np.float32(s1)))
            v = v * s1 + x64
            e = (e + 32 * U32 * mag + (K + 40) * U32 * np.abs(x64 * inv)) * abs(s1) + np.abs(x64) * abs(inv * float(np.float32(s1)) - 1.0)
        e = e + round16(v)  # the staged tile
        for which, s in (("res1", s1), ("res2", s2)):
            if args.get(which) is None:
                continue
            r = np.asarray(args[which])[out_index(args, which)].astype(np.float64)
            scaled = not (s1 == 1.0 and s2 == 1.0)
            f32_ops = 2 * U32 * (np.abs(v * s) + np.abs(r)) if scaled else 0.0
            v = v * s + r
            e = e * abs(s) + f32_ops + round16(v)
        idx = out_index(args)
        assert np.unique(idx).size == idx.size and idx.max() < size
        want[idx], allow[idx], written[idx] = v, e, True
    return {"out": want}, {"out": allow}, {"out": written}

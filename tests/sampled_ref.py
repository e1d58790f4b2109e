"""float64 references of the sampling and halo matrix-core kernels -- vx_deform_conv_f16, vx_bf_deform_cols_f16, vx_mbconv_dw_pw_f16,
vx_conv3x3_f16 -- and derived per-element error allowances. Plain numpy, nothing from the device side. What tests/deform_ref.py (the sampler),
tests/gemm_ref.py (the halo conv is a vx_gemm_args call), tests/dconv_ref.py (round16, the accumulation term) and tests/graph_ref.py (the GELU
bound) already derive is imported.

`evaluate(entry, args, guard)` -> (want, allow, written): flat arrays over the WHOLE output buffer -- what lies in front of `out` (`out_off`
elements), the call's rows, then `guard` elements -- as the call leaves a zero-initialised one: the expected content (float64), the allowance of
every element (float64) and which elements the call writes (bool). An element the call must not write has allowance 0, so `|got - want| <=
allowance` also catches a stray store. The guard is at least one full tile of the kernel (`min_guard`).

entry "deform" (vx_deform_conv_f16); args: x f16 [B, H, W, Cin]; w f16 [Cout pad 32, k k Cin]; offset f16 [M, ld_offset] (the whole buffer: in
  mask mode 2 it may hold the logits too, `mask_col` = their first column, and then `mask` is None); mask f16 [M, ld_mask] or None; mask_mode,
  mask_scale; scale, bias f32 [Cout] or None; relu; k, pad, Cout, ldo, out_off. out f16 [M, ldo], columns < Cout written:
  relu?(scale * sum_t,c mask[t] sample_t(x)[c] w[n, t, c] + bias), M = B OH OW, OH = H + 2 pad - k + 1.
entry "cols" (vx_bf_deform_cols_f16); args: x f16 [B, h, w, C]; om f16 [M, ldom] (2 taps offsets, taps logits); k (pad k / 2).
  out f16 [M, taps C] = 2 sigmoid(logit[t]) sample_t(x).
entry "mbconv" (vx_mbconv_dw_pw_f16); args: h f16 [B, H, W, 256]; w2 f16 [9, 256]; b2 f32 [256]; w3_rows f16 [64, 256] (and `w3`, its
  vx_mbconv_pack_w3 image, which the reference does not read); b3 f32 [64]; x f16 [B, H, W, 64].
  out f16 [B, H, W, 64] = gelu(x + gelu(dw3x3(h) + b2) @ w3^T + b3).
entry "halo" (vx_conv3x3_f16); args: the dict of tests/gemm_ref.py; `guard` must be whole rows of ldo elements.

The allowances (u16 = 2^-11, u32 = 2^-24), from the arithmetic only, never from device output:
  the sampler (deform, cols), per A element. The position is the reference's own f32 sum, so floor, ly = py - floor(py) and lx are the device's
            (the subtraction is exact). Counted from the source text, in the form with the most roundings (nothing contracted): a weight is
            (1 - ly) * (1 - lx): three roundings, relative to its own term; the product with the corner value: one; the three adds of the blend:
            one each, on partial sums; the product with the mask: one. The weights sum to 1, so with V = the largest magnitude among the corners
            that count every one of these 3 + 1 + 3 + 1 = 8 roundings is at most u32 V |mask|; one spare unit pays for the second-order terms:
            SAMPLER_ROUNDINGS = 9 u32 V |mask|. Then ONE f16 rounding of the product, round16. A sample with no corner inside is exactly 0.
            Mask mode 2 and `cols` form the mask as s / (1 + __expf(-logit)): by the project's convention (attn_ref.py, gemm_ref.py) an exp-based
            term has no documented bound here and gets F16_TOL = 4e-3 of the largest reference magnitude of the call, added to every written
            element. Modes 0 and 1 keep the sharp bound.
  deform    the A term pushed through |w|; (taps Cin + 8) u32 (|a| (*) |w| |scale| + |bias|) for the any-order f32 accumulation, the 8 spare
            units paying for the multiplication by scale and the bias add; everything carried times |scale|; one round16 on the way out. A
            ReLU whose argument lies below zero by more than its own bound is exactly 0 on the device as well: allowance 0.
  cols      the A term alone.
  mbconv    depthwise: (9 + 8) u32 (|h| (*) |w2| + |b2|). The inner GELU is vx_device.h's gelu_tanh, which graph_ref.GELU_F16_ULPS bounds: its f16
            result is within 1 f16 ulp of the float64 GELU of the SAME argument rounded to f16 (half an ulp more); the argument's error is
            multiplied by GELU's Lipschitz constant (< 1.13). That pushed through |w3|, plus (256 + 8) u32 (|d| (*) |w3| + |b3| + |x|); the
            outer GELU is bounded the same way.
  halo      gemm_ref's allowance, as it is."""
from __future__ import annotations

import numpy as np

import deform_ref as D
import gemm_ref as G
from dconv_ref import U16, U32, accumulation_term, round16  # noqa: F401
from graph_ref import GELU_F16_ULPS, f16_ulp

F16_TOL = G.F16_TOL
SAMPLER_ROUNDINGS = 9
GELU_LIPSCHITZ = 1.13
DEFORM_TILE = 64  # output pixels per block of the deformable conv
MB_C, MB_CO, MB_PX = 256, 64, 64


def f64(a):
    return np.asarray(a, np.float64)


def min_guard(entry: str, args) -> int:
    """elements of one full tile of the kernel behind the last row"""
    if entry == "deform":
        return DEFORM_TILE * args["ldo"]
    if entry == "cols":
        return 256 * 8  # one block of 16-byte stores
    if entry == "mbconv":
        return MB_PX * MB_CO
    ldo = 1 if args["epi"] == G.HEAD_OUT else args["ldo"]
    return 8 * (-(-args["conv_W"] // 32) * 32) * ldo  # the 8 x 32 tile's rows below the map


# ---- operand layouts -----------------------------------------------------------------------------------------------------------------------

def pack_w3(rows: np.ndarray) -> np.ndarray:
    """W3 [64][256] -> the fragment order of the header: out[((nt * 16 + s) * 64 + lane) * 8 + j] = W3[32 nt + (lane & 31)][(2 s + (lane >> 5)) * 8 + j]"""
    t = np.asarray(rows).reshape(2, 32, 16, 2, 8)  # [nt][m][s][hh][j]
    return np.ascontiguousarray(t.transpose(0, 2, 3, 1, 4)).reshape(-1)  # [nt][s][hh][m][j]: lane = 32 hh + m


def unpack_w3(packed: np.ndarray) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(packed).reshape(2, 16, 2, 32, 8).transpose(0, 3, 1, 2, 4)).reshape(64, 256)


def mbconv_block(b, nwg):
    """the kernel's XCD-aware order: hardware block b of a grid of nwg -> the row segment it computes"""
    b = np.asarray(b)
    q, rem, xcd = nwg >> 3, nwg & 7, b & 7
    return np.where(xcd < rem, xcd * (q + 1), rem * (q + 1) + (xcd - rem) * q) + (b >> 3)


# ---- the sampler -------------------------------------------------------------------------------------------------------------------------------

def gelu(x):
    return G.gelu_tanh(x)


def deform_mask(args):
    """-> (offsets [B, OH, OW, 2 taps], the mask factor [B, OH, OW, taps] or None, whether it is exp-based)"""
    B, H, W, k, pad = (args[key] for key in ("B", "H", "W", "k", "pad"))
    taps, OH, OW = k * k, H + 2 * pad - k + 1, W + 2 * pad - k + 1
    om = np.asarray(args["offset"])
    off = f64(om[:, :2 * taps]).reshape(B, OH, OW, 2 * taps)
    mode = args["mask_mode"]
    if mode == 0:
        return off, None, False
    raw = om[:, args["mask_col"]:args["mask_col"] + taps] if args.get("mask") is None else np.asarray(args["mask"])[:, :taps]
    raw = f64(raw).reshape(B, OH, OW, taps)
    if mode == 1:
        return off, raw, False
    return off, float(np.float32(args["mask_scale"])) * D.sigmoid(raw), True


def _a_term(cols, big):
    """the device's error on an A element: the f32 blend and the one f16 rounding; exactly 0 where no corner counts"""
    return np.where(big > 0, SAMPLER_ROUNDINGS * U32 * big + round16(cols), 0.0)


def deform(args):
    """-> (want, allow) [M, Cout] and the A operand [M, taps Cin]"""
    x, k, pad, Cout = f64(args["x"]), args["k"], args["pad"], args["Cout"]
    off, mask, exp_based = deform_mask(args)
    cols, big = D.deform_columns(x, off, k, k, pad, mask)
    M, K = off.shape[0] * off.shape[1] * off.shape[2], k * k * x.shape[3]
    a, ea = cols.reshape(M, K), _a_term(cols, big).reshape(M, K)
    w = f64(args["w"])[:Cout]
    assert w.shape == (Cout, K)
    scale = np.ones(Cout) if args.get("scale") is None else f64(args["scale"])
    bias = np.zeros(Cout) if args.get("bias") is None else f64(args["bias"])
    v = (a @ w.T) * scale + bias
    e = (ea @ np.abs(w).T) * np.abs(scale) + accumulation_term(K, (np.abs(a) @ np.abs(w).T) * np.abs(scale) + np.abs(bias))
    if exp_based:
        e = e + F16_TOL * np.abs(np.maximum(v, 0.0) if args.get("relu") else v).max()
    if args.get("relu"):
        clipped = v + e < 0
        v = np.maximum(v, 0.0)
        return v, np.where(clipped, 0.0, e + round16(v)), a
    return v, e + round16(v), a


def cols(args):
    """-> (want, allow) [M, taps C]"""
    x, k = f64(args["x"]), args["k"]
    B, h, w, C = x.shape
    taps = k * k
    om = f64(np.asarray(args["om"])[:, :3 * taps])
    off, logit = om[:, :2 * taps].reshape(B, h, w, 2 * taps), om[:, 2 * taps:].reshape(B, h, w, taps)
    c, big = D.deform_columns(x, off, k, k, k // 2, 2.0 * D.sigmoid(logit))
    want = c.reshape(B * h * w, taps * C)
    return want, _a_term(c, big).reshape(want.shape) + F16_TOL * np.abs(want).max()


# ---- mbconv ------------------------------------------------------------------------------------------------------------------------------------

def depthwise3x3(h, w2):
    """h [B, H, W, C], w2 [9, C], zero padding 1"""
    B, H, W, C = h.shape
    hp = np.pad(h, ((0, 0), (1, 1), (1, 1), (0, 0)))
    out = np.zeros_like(h)
    for t in range(9):
        ky, kx = divmod(t, 3)
        out += hp[:, ky:ky + H, kx:kx + W] * w2[t]
    return out


def gelu_f16_term(v, e):
    """the f16 result of the device's GELU of an argument known to e: the float64 GELU v carries 1.13 e, its rounding to f16 half an ulp, the
    device's own result up to GELU_F16_ULPS more (ulps taken at the largest magnitude the value can have)"""
    carried = GELU_LIPSCHITZ * e
    top = np.abs(v) + carried
    return carried + round16(top) + GELU_F16_ULPS * f16_ulp(top * (1 + 2 * U16))


def mbconv(args):
    """-> (want, allow) [B, H, W, 64] and the reference's depthwise output"""
    h, w2, b2 = f64(args["h"]), f64(args["w2"]), f64(args["b2"])
    w3, b3, x = f64(args["w3_rows"]), f64(args["b3"]), f64(args["x"])
    d = depthwise3x3(h, w2) + b2
    ed = accumulation_term(9, depthwise3x3(np.abs(h), np.abs(w2)) + np.abs(b2))
    g = gelu(d)
    eg = gelu_f16_term(g, ed)
    z = g @ w3.T + b3 + x
    ez = eg @ np.abs(w3).T + accumulation_term(MB_C, np.abs(g) @ np.abs(w3).T + np.abs(b3) + np.abs(x))
    y = gelu(z)
    return y, gelu_f16_term(y, ez), d


# ---- evaluate ------------------------------------------------------------------------------------------------------------------------------------

def _rows(want, allow, ldo, out_off, guard):
    """[M, n] values in rows of ldo elements behind out_off elements, guard elements after the last row"""
    M, n = want.shape
    size = out_off + M * ldo + guard
    full_w, full_a, written = np.zeros(size), np.zeros(size), np.zeros(size, bool)
    idx = out_off + np.arange(M)[:, None] * ldo + np.arange(n)[None, :]
    full_w[idx], full_a[idx], written[idx] = want, allow, True
    return full_w, full_a, written


def evaluate(entry: str, args, guard: int):
    if entry == "deform":
        want, allow, _ = deform(args)
        return _rows(want, allow, args["ldo"], args.get("out_off", 0), guard)
    if entry == "cols":
        want, allow = cols(args)
        return _rows(want, allow, want.shape[1], 0, guard)
    if entry == "mbconv":
        want, allow, _ = mbconv(args)
        return _rows(want.reshape(-1, MB_CO), allow.reshape(-1, MB_CO), MB_CO, 0, guard)
    assert entry == "halo"
    ldo = 1 if args["epi"] == G.HEAD_OUT else args["ldo"]
    assert guard % ldo == 0
    want, allow, written = G.evaluate(args, guard // ldo)
    return want["out"].reshape(-1), allow["out"].reshape(-1), written["out"].reshape(-1)

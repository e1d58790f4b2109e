"""float64 references of the row kernels around the matrix-core kernels -- the LayerNorms of csrc/kernels_misc.hip, kernels_tinyvit.hip and
kernels_swin.hip, the two window reverse + residual adds, the depthwise 3x3 and the two elementwise helpers -- with a per-element allowance
derived from the arithmetic, never from device output. Plain numpy, nothing from the device side.

`evaluate(entry, args, guard)` -> (want, allow, written) over the WHOLE output buffer (flat; the rows, what lies between them, and `guard`
elements behind the last row) as the call leaves a buffer that started filled with CANARY. Zero is an expected value here (the SWIN pad rows),
so the buffer is not zero-initialised: CANARY = -24000 is finite, exact in f16 and f32, and nothing here comes near it (the LayerNorm, add and
depthwise cases on ordinary data stay below 1e3, a GELU is never below -0.17 and the large-magnitude cases hold nothing between 40 and
30000 in magnitude; tests/test_rows_ref_cpu.py asserts that every element a call writes lies further from it than its allowance plus 1000). An element the call must not
write has `written` False, allowance 0 and must still hold the canary's bits (tests/buffer_check.py, with `untouched=CANARY`). `min_guard` is one full block of the kernel's rows.

Entries (`args` holds the launcher's own arguments, numpy arrays for the whole operands, already rounded to the type the kernel reads):
  ln32          vx_layernorm_f32_f16             x f32 [M, C] -> f16 [M, C]
  tv_ln         vx_layernorm_f16                 x f16 [B res res | rows, C] -> f16 / f32 [rows_out, C]; ws > 0: window order, pad rows = bias
  swin_ln       vx_swin_layernorm_f16            x f16 [B H W | rows, C] -> [rows_out, C]; ws > 0: pad + roll(-shift) + partition, pad rows = 0
  swin_ln_strided  vx_swin_layernorm_strided_f16 plain rows, output rows of ldy elements
  swin_merge    vx_swin_merge_layernorm_f16      x f16 [B, H, W, C] -> f16 [B H/2 W/2, 4 C]
  swin_reverse  vx_swin_window_reverse_add_f16   y[pixel] = x[pixel] + a[its window row]
  tv_reverse    vx_window_reverse_add_f16        the same on a square map without shift
  dwconv        vx_dwconv3x3_f16                 3x3, pad 1, stride 1 | 2, + bias, optional GELU
  add_gelu      vx_add_gelu_f16                  gelu(a + b), b may be None
  add_rows      vx_add_rows_f16                  a (f16 | f32) + b[i mod period]

The window mappings are written once here from the reference's text (swin.cpp:48-76, 117-161: pad, roll, partition, reverse, crop, the 2 x 2
gather of patch merging; mobile-sam.cpp:25-64): `partition_rows` gives, for every output row of a window-ordered buffer, the pixel it reads
(-1: padding), `reverse_rows` the window row every pixel reads back, `merge_gather` the four pixels of a merged row in the reference's concat
order (y even x even | y odd x even | y even x odd | y odd x odd).

The allowances (u16 = 2^-11, u32 = 2^-24):
  LayerNorm  block_ref.layer_norm's derivation (mean, centred values, variance, rstd, value; it grows for rows whose mean dwarfs their spread)
             with the row width for its D and no incoming error, plus round16 of the result for f16 output and one u32 |want| for f32 output.
             The rstd term is the kernel's: kernels_misc.hip and kernels_tinyvit.hip use v_rsq_f32 (block_ref.RSQ_REL, an ASSUMED figure);
             kernels_swin.hip divides 1 by sqrtf, and the build (-O3, no fast-math option) makes both correctly rounded -- the assembly holds
             the v_div_scale / v_div_fmas / v_div_fixup sequence and a refined v_sqrt_f32, no v_rsq_f32 -- so there it is two f32 roundings.
             The rstd bound |(1 + t)^-1/2 - 1| <= t / 2 + t^2 holds up to t = 0.6 on the side where the variance is underestimated;
             `layer_norm_rows` asserts t <= 0.6 for every row but the constant ones, whose centred values are zero.
             Pad rows carry no arithmetic: SWIN writes zeros, TinyViT 0 rstd g + b = b exactly: allowance 0.
  adds       f16 + f16 in f32 and one rounding to f16: f32's 24 bits are 2 x 11 + 2, so the double rounding is the single one: allowance 0,
             bit equality with f16(a + b) of float64. With an f32 operand the f32 sum rounds: u32 |s|, then round16.
  depthwise  (9 + 8) u32 (|x| (*) |w| + |b|) on the sum; without GELU round16 on top.
  GELU       as tests/sampled_ref.py bounds vx_device.h's gelu_tanh: 1.13 times the argument's error, half an f16 ulp for the rounding,
             graph_ref.GELU_F16_ULPS for the device's exp2 / rcp."""
from __future__ import annotations

import numpy as np

import block_ref as B
from block_ref import U16, U32, round16  # noqa: F401
from dconv_ref import accumulation_term
from graph_ref import gelu
from sampled_ref import gelu_f16_term

CANARY = -24000.0
SQRT_DIV_REL = 2 * U32  # 1.0f / sqrtf(v), both correctly rounded
RSTD_REL = {"ln32": B.RSQ_REL, "tv_ln": B.RSQ_REL, "swin_ln": SQRT_DIV_REL, "swin_ln_strided": SQRT_DIV_REL, "swin_merge": SQRT_DIV_REL}
T_LIMIT = 0.6


def f64(a):
    return np.asarray(a).astype(np.float64)


def f16(a):
    with np.errstate(over="ignore"):
        return np.asarray(a, np.float64).astype(np.float16).astype(np.float64)


# ---- the launchers' row groups, restated (rows per block of 256 threads) --------------------------------------------------------------------

def tv_ln_rows_per_block(C) -> int:
    return 16 if C <= 128 else 8 if C <= 256 else 4


def swin_ln_lanes(C):
    """(lanes per row, chunks per lane) of vx_swin_layernorm_f16; vx_swin_merge_layernorm_f16 takes it at 4 C (up to (64, 8))"""
    return (16, 1) if C <= 128 else (32, 1) if C <= 256 else (64, 1) if C <= 512 else (64, 2) if C <= 1024 else (64, 4) if C <= 2048 else (64, 8)


def dwconv_extent(H, W, stride):
    return (H + 2 - 3) // stride + 1, (W + 2 - 3) // stride + 1


def min_guard(entry: str, a) -> int:
    """one full block of the kernel's rows behind the last row, in elements"""
    if entry == "ln32":
        return 4 * a["C"]
    if entry == "tv_ln":
        return tv_ln_rows_per_block(a["C"]) * a["C"]
    if entry in ("swin_ln", "swin_ln_strided"):
        return (256 // swin_ln_lanes(a["C"])[0]) * (a.get("ldy") or a["C"])
    if entry == "swin_merge":
        return (256 // swin_ln_lanes(4 * a["C"])[0]) * 4 * a["C"]
    if entry == "dwconv":
        return 256 * 8 * (8 if a["stride"] == 1 else 4)  # 256 threads of P pixels x 8 channels
    return 256 * 8


# ---- the window mappings ------------------------------------------------------------------------------------------------------------------------

def partition_rows(Bn, H, W, ws, shift=0):
    """pad to whole windows, roll(-shift), window_partition (swin.cpp:48-56, 108-119; mobile-sam.cpp:32-43) on the pixel indices:
    -> int64 [B nwy nwx ws ws], the pixel (b H + y) W + x every window row reads, -1 where the padded map has no pixel"""
    hp, wp = -(-H // ws) * ws, -(-W // ws) * ws
    p = np.full((Bn, hp, wp), -1, np.int64)
    p[:, :H, :W] = np.arange(Bn * H * W).reshape(Bn, H, W)
    if shift > 0:
        p = np.roll(p, (-shift, -shift), (1, 2))
    return p.reshape(Bn, hp // ws, ws, wp // ws, ws).transpose(0, 1, 3, 2, 4).reshape(-1)


def reverse_rows(Bn, H, W, ws, shift=0):
    """window_reverse, roll(+shift), crop (swin.cpp:58-67, 121-131; mobile-sam.cpp:54-63) on the window row indices: -> int64 [B H W], the
    window row every pixel takes its value from"""
    hp, wp = -(-H // ws) * ws, -(-W // ws) * ws
    nwy, nwx = hp // ws, wp // ws
    r = np.arange(Bn * hp * wp).reshape(Bn, nwy, nwx, ws, ws).transpose(0, 1, 3, 2, 4).reshape(Bn, hp, wp)
    if shift > 0:
        r = np.roll(r, (shift, shift), (1, 2))
    return r[:, :H, :W].reshape(-1)


def merge_gather(Bn, H, W):
    """patch_merging's concat of four strided slices (swin.cpp:148-156): -> int64 [B H/2 W/2, 4], the pixels of every merged row in concat
    order: (y even, x even), (y odd, x even), (y even, x odd), (y odd, x odd)"""
    idx = np.arange(Bn * H * W).reshape(Bn, H, W)
    parts = [idx[:, 0::2, 0::2], idx[:, 1::2, 0::2], idx[:, 0::2, 1::2], idx[:, 1::2, 1::2]]
    return np.stack([p.reshape(-1) for p in parts], axis=1)


# ---- LayerNorm ------------------------------------------------------------------------------------------------------------------------------------

def layer_norm_rows(x, g, b, eps, rsq_rel, out_f32):
    """x [rows, C] float64 (exact inputs) -> (want, allow) of the stored value"""
    info = {}
    want, allow = B.layer_norm(x, np.zeros_like(x), f64(g), f64(b), float(eps), width=x.shape[1], rsq_rel=rsq_rel, info=info)
    spread = np.ptp(x, axis=1) > 0
    assert (info["t"][spread] <= T_LIMIT).all(), "a row outside the range the rstd bound is valid on"
    return want, allow + (U32 * np.abs(want) if out_f32 else round16(np.abs(want) + allow))


def out_round(v, out_f32):
    return f64(np.asarray(v, np.float32)) if out_f32 else f16(v)


def layer_norm_source(entry, a):
    """-> (x [rows_out, C] float64 as the kernel gathers it (zeros in pad rows), pad [rows_out] bool)"""
    C = a["C"]
    if entry == "ln32":
        return f64(a["x"]).reshape(a["M"], C), np.zeros(a["M"], bool)
    if entry == "swin_merge":
        x = f64(a["x"]).reshape(-1, C)
        return x[merge_gather(a["B"], a["H"], a["W"])].reshape(-1, 4 * C), np.zeros(a["B"] * (a["H"] // 2) * (a["W"] // 2), bool)
    x = f64(a["x"]).reshape(-1, C)
    if not a.get("ws"):
        assert x.shape[0] == a["rows_out"]
        return x, np.zeros(x.shape[0], bool)
    src = partition_rows(a["B"], a["res"], a["res"], a["ws"]) if entry == "tv_ln" else partition_rows(a["B"], a["H"], a["W"], a["ws"], a["shift"])
    assert src.size == a["rows_out"]
    return np.where((src < 0)[:, None], 0.0, x[np.maximum(src, 0)]), src < 0


def layer_norm_entry(entry, a):
    """-> (want, allow, pad) [rows_out, width]"""
    x, pad = layer_norm_source(entry, a)
    out_f32 = bool(a.get("out_f32"))
    want, allow = layer_norm_rows(x, a["w"], a["b"], a["eps"], RSTD_REL[entry], out_f32)
    if pad.any():
        want[pad] = out_round(f64(a["b"]), out_f32) if entry == "tv_ln" else 0.0  # TinyViT pads before the norm, SWIN after it
        allow[pad] = 0.0
    return want, allow, pad


def zero_bit_elements(entry, a, size):
    """the elements of the flat output that must hold zero BITS (the SWIN pad rows: +0, not -0)"""
    out = np.zeros(size, bool)
    if entry == "swin_ln" and a.get("ws"):
        pad = layer_norm_source(entry, a)[1]
        C = a["C"]
        out[:pad.size * C] = np.repeat(pad, C)
    return out


# ---- the other entries ----------------------------------------------------------------------------------------------------------------------------

def reverse_add(entry, a):
    C = a["C"]
    H, W, shift = (a["res"], a["res"], 0) if entry == "tv_reverse" else (a["H"], a["W"], a["shift"])
    rows = reverse_rows(a["B"], H, W, a["ws"], shift)
    want = f16(f64(a["x"]).reshape(-1, C) + f64(a["a"]).reshape(-1, C)[rows])
    return want, np.zeros_like(want)


def depthwise3x3(x, w, stride):
    """x [B, H, W, C], w [9, C], zero padding 1 -> [B, OH, OW, C]"""
    Bn, H, W, C = x.shape
    OH, OW = dwconv_extent(H, W, stride)
    xp = np.pad(x, ((0, 0), (1, 1), (1, 1), (0, 0)))
    out = np.zeros((Bn, OH, OW, C))
    for t in range(9):
        ky, kx = divmod(t, 3)
        out += xp[:, ky:ky + (OH - 1) * stride + 1:stride, kx:kx + (OW - 1) * stride + 1:stride] * w[t]
    return out


def dwconv(a):
    x, w, b = f64(a["x"]), f64(a["w"]), f64(a["bias"])
    s = depthwise3x3(x, w, a["stride"]) + b
    e = accumulation_term(9, depthwise3x3(np.abs(x), np.abs(w), a["stride"]) + np.abs(b))
    if a["gelu"]:
        v = gelu(s)
        return v, gelu_f16_term(v, e)
    return s, e + round16(np.abs(s) + e)


def add_gelu(a):
    s = f64(a["a"]) + (0.0 if a["b"] is None else f64(a["b"]))
    v = gelu(s)
    return v, gelu_f16_term(v, U32 * np.abs(s))


def add_rows(a):
    n, period = a["n"], a["period"]
    s = f64(a["a"]).reshape(-1) + f64(a["b"]).reshape(-1)[np.arange(n) % period]
    if a["a_is_f32"]:
        e = U32 * np.abs(s)
        return s, e + round16(np.abs(s) + e)
    return f16(s), np.zeros(n)


# ---- evaluate -------------------------------------------------------------------------------------------------------------------------------------

def _buffer(want, allow, ld, guard):
    """[rows, n] values in rows of ld elements, guard elements behind the last row; everything else keeps the canary"""
    rows, n = want.shape
    size = rows * ld + guard
    full_w, full_a, written = np.full(size, CANARY), np.zeros(size), np.zeros(size, bool)
    idx = np.arange(rows)[:, None] * ld + np.arange(n)[None, :]
    full_w[idx], full_a[idx], written[idx] = want, allow, True
    return full_w, full_a, written


LAYER_NORMS = ("ln32", "tv_ln", "swin_ln", "swin_ln_strided", "swin_merge")


def out_dtype(entry, args):
    return np.float32 if entry in ("tv_ln", "swin_ln", "swin_ln_strided") and args.get("out_f32") else np.float16


def canary_buffer(size, dtype):
    """what an output buffer holds before the call: buffer_check.violations(got, ref, untouched=CANARY) is the comparison"""
    return np.full(size, CANARY, dtype)


def evaluate(entry: str, args, guard: int):
    assert guard >= min_guard(entry, args)
    if entry in LAYER_NORMS:
        want, allow, _ = layer_norm_entry(entry, args)
        return _buffer(want, allow, (args.get("ldy") or want.shape[1]) if entry == "swin_ln_strided" else want.shape[1], guard)
    if entry in ("swin_reverse", "tv_reverse"):
        want, allow = reverse_add(entry, args)
    elif entry == "dwconv":
        want, allow = dwconv(args)
    elif entry == "add_gelu":
        want, allow = add_gelu(args)
    else:
        assert entry == "add_rows"
        want, allow = add_rows(args)
    want, allow = want.reshape(1, -1), allow.reshape(1, -1)
    return _buffer(want, allow, want.shape[1], guard)

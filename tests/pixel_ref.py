"""float64 references of the image entry and exit kernels -- what turns a u8 image into the first tensor of a family and the last tensor back into
an image: csrc/kernels_misc.hip (patches, plain f32, cls rows, head output, min/max normalisation, f32 -> u8), kernels_tinyvit.hip (value +
residue pixels, sam::interpolate_bilinear) and kernels_birefnet.hip (half-size value + residue pixels, image_to_patches) -- with a per-element
allowance derived from the kernel's rounding steps, never from device output. Plain numpy, nothing from the device side.

`evaluate(entry, args, guard, got=None)` -> (want, allow, written) over the WHOLE output buffer (flat: the values and `guard` elements behind the
last one) as the call leaves a buffer that started filled with CANARY (CANARY_U8 for a u8 output; the prior contents for the in-place
vx_write_cls_rows). Zero is an expected value here (pad columns, the minimum of an image), so no buffer is zero-initialised. A u8 output is
compared byte for byte (`u8_violations`, the u8 twin of buffer_check.violations: the same three verdicts on bytes, allowance 0 everywhere).

Entries (`args` holds the launcher's arguments, numpy arrays for the whole operands in the type the kernel reads):
  patches    vx_preprocess_patches   rgb u8 [B, H, W, 3] -> f16 [B ph pw, Kp], k = (ky ps + kx) 3 + c, columns [3 ps ps, Kp) zero
  pre32      vx_preprocess_f32       rgb u8 [B, H, W, 3] -> f32 [B, H, W, 3]
  cls        vx_write_cls_rows       x f32 [B T, C] in place: row b T = cls + pos[:C]
  head_out   vx_head_out_f32         x f16 [n, C], w f32 [C] -> f32 [n]: max_depth relu(x . w + bias)
  minmax     vx_minmax_normalize     d f32 [B, n] -> f32 [B, n], every image by its own extremes
  u8         vx_f32_to_u8            f32 [n] -> u8 [n]: uint8(fl32(clamp(v, 0, 1) 255))
  tvpre      vx_tv_preprocess        rgb u8 [n, 3] -> f16 [n, 8]: value | residue | 0 0
  bfhalf     vx_bf_preprocess_half   rgb u8 [B, H, W, 3] -> f16 [B, H/2, W/2, 8], bilinear align_corners, value | residue | 0 0
  bfpatches  vx_bf_patches           rgb u8 [B, gh h, gw w, 3] -> f16 [B, h, w, 3 gw gh], channel gx + gw (gy + gh c)
  sam        vx_sam_interpolate      f16 column of a [pixels][8] buffer | f32 rows of sstride -> f32 | u8 [dh, dw], half-pixel centres

The allowances (u16 = 2^-11, u32 = 2^-24, TINY16 = half the f16 subnormal step; SLACK = 1 + 2^-20 covers the products of two error terms):
  normalisation by division  p = (u / 255 - m) s with q = u / 255, d = q - m: three f32 roundings (IEEE division, difference, product; m and s
             are the f32 values the caller hands in, exact): u32 (|q| |s| + |d| |s| + |p|). The f16 table of vx_preprocess_patches and the value
             channels of vx_tv_preprocess add round16(|p| + that).
  normalisation by product   kernels_birefnet.hip multiplies by the f32 constant 1 / 255 (relative error u32) where the contract divides: one more
             unit on q: u32 (2 |q| |s| + |d| |s| + |p|); a contracted multiply-add only removes a rounding.
  residue    channel 3 + c holds f16(v - hi) of the f32 value v and ITS OWN stored f16 hi; v - hi is exact in f32 (hi is v's neighbour). So
             the reference of a residue is p - hi with the hi the buffer under test holds (`got`): allowance = the f32 allowance of v plus
             round16(|p - hi| + that): hi + residue reconstructs the float64 value to f32 accuracy plus the residue's own rounding.
  bilinear, align_corners (vx_bf_preprocess_half)   the source coordinate o ((n - 1) / (on - 1)) carries two f32 roundings: |df| <= 2 u32 f. The
             interpolant is continuous and piecewise linear, so a coordinate error moves the value by at most df times the steepest slope of the
             cells it can reach: the largest difference of vertical (horizontal) neighbours among source rows y0 - 1 .. y0 + 2 and columns
             x0 - 1 .. x0 + 2. Each lerp a + (b - a) t is three roundings on |b - a| <= 2 M, |(b - a) t| <= 2 M, and the result <= M: 5 u32 M;
             two levels: 10 u32 M (M the largest of the four taps' magnitudes), plus the largest of the taps' normalisation allowances.
  cls rows   one f32 add: bit equal to numpy's float32 sum, allowance 0; every other row keeps its prior bits.
  head out   C products and C sums in f32 (contracted or not) and the bias: (2 C + 1) u32 (|x| . |w| + |bias|) on z; times |max_depth| plus
             u32 |want| for the last product. Where z lies below minus that, the ReLU gives +0 whatever the roundings did: allowance 0, zero bits.
  min/max    the extremes are exact (comparisons). delta = fl(max - min), scale = fl(1 / delta), offset = fl(-min scale), out =
             fl(fl(d scale) + offset): the two roundings of scale act on (d - min) / delta = want, the two products on |d| s and |min| s, the sum on
             want: u32 (3 |want| + (|d| + |min|) s). fl(min scale) + fl(-min scale) is +0.0 exactly: the minimum of every image has
             allowance 0 and zero bits. delta < 1e-5 (decided on the f32 difference, as the kernel does): scale 1, out = fl(d - min): u32 |want|.
  f32 -> u8  no allowance: byte equal to the float32 evaluation of the contract in numpy (np.fmax sends NaN to 0 as fmaxf does).
  sam        coordinates and weights in numpy float32 exactly as the kernel states them (contraction is off there); the blend in float64. Each
             level (1 - w) a + w b rounds 1 - w (u32 |a|), two products (u32 (|(1 - w) a| + |w b|) <= u32 M) and the sum (u32 M): 3 u32 M; two
             levels: 6 u32 M. A u8 output is 255 where the value is positive: a value within its allowance of 0 is undecided (`sam_undecided`);
             the case table holds none (tests/test_pixel_ref_cpu.py), so the device owes byte equality."""
from __future__ import annotations

import numpy as np

from block_ref import TINY16, U16, U32, round16  # noqa: F401

CANARY = -24000.0      # finite, exact in f16 and f32; no case writes a value within 1000 of it (tests/test_pixel_ref_cpu.py)
CANARY_U8 = 0xA5       # neither 0 nor 255; the f32 -> u8 table writes it too, which only a stray store of the same byte could hide behind
SLACK = 1.0 + 2.0 ** -20
F32 = np.float32
IMAGENET_MEAN = np.array([0.485, 0.456, 0.406], F32)
IMAGENET_STD = np.array([0.229, 0.224, 0.225], F32)
IMAGENET_INV = F32(1.0) / IMAGENET_STD  # 1.0f / 0.229f ..., folded by the compiler in f32 (correctly rounded)
GRID_CAP, BLOCK = 4096, 256  # grid_stride_blocks(n, 256 * 16): the three grid-stride kernels
U8_ENTRIES = ("u8",)
RESIDUE_ENTRIES = ("tvpre", "bfhalf")


def f64(a):
    return np.asarray(a).astype(np.float64)


def f16(a):
    return np.asarray(a, np.float64).astype(np.float16).astype(np.float64)


# ---- the normalisations ---------------------------------------------------------------------------------------------------------------------

def norm_div(u, mean, inv):
    """(u / 255 - mean) * inv for u [..., 3] -> (p, its f32 allowance)"""
    m, s = f64(mean), f64(inv)
    q = f64(u) / 255.0
    d = q - m
    p = d * s
    return p, U32 * (np.abs(q) * np.abs(s) + np.abs(d) * np.abs(s) + np.abs(p)) * SLACK


def norm_mul(u):
    """kernels_birefnet.hip's norm_px against the contract (u / 255 - mean) / std -> (p, its f32 allowance)"""
    m, s = f64(IMAGENET_MEAN), f64(IMAGENET_INV)
    q = f64(u) / 255.0
    d = q - m
    p = d * s
    return p, U32 * (2 * np.abs(q) * np.abs(s) + np.abs(d) * np.abs(s) + np.abs(p)) * SLACK


def residue_pixels(v, e32, hi=None):
    """v, e32 [n, 3] -> (want, allow) [n, 8]: value | residue against the stored hi (default: the float64 value's own rounding) | 0 0"""
    n = v.shape[0]
    want, allow = np.zeros((n, 8)), np.zeros((n, 8))
    want[:, :3], allow[:, :3] = v, e32 + round16(np.abs(v) + e32)
    hi = f16(v) if hi is None else f64(hi)
    with np.errstate(invalid="ignore"):
        r = np.where(np.isfinite(hi), v - hi, 0.0)  # (a non-finite hi is rejected on its own channel)
    want[:, 3:6], allow[:, 3:6] = r, e32 + round16(np.abs(r) + e32)
    return want, allow


# ---- the entries -----------------------------------------------------------------------------------------------------------------------------

def patches(a):
    B, H, W, ps, Kp = (a[k] for k in ("B", "H", "W", "ps", "Kp"))
    ph, pw, kreal = H // ps, W // ps, ps * ps * 3
    p, e = norm_div(a["rgb"].reshape(B, H, W, 3), a["mean"], a["inv"])

    def rows(t):  # k = (ky, kx, c) of patch (py, px)
        return t.reshape(B, ph, ps, pw, ps, 3).transpose(0, 1, 3, 2, 4, 5).reshape(B * ph * pw, kreal)
    want, allow = np.zeros((B * ph * pw, Kp)), np.zeros((B * ph * pw, Kp))
    want[:, :kreal] = rows(p)
    allow[:, :kreal] = rows(e + round16(np.abs(p) + e))
    return want, allow


def pre32(a):
    return norm_div(a["rgb"].reshape(-1, 3), a["mean"], a["inv"])


def cls_rows(a):
    """-> (want, allow, written) [B T, C]: the prior rows, row b T replaced by the float32 sum"""
    B, T, C = a["B"], a["T"], a["C"]
    x = a["x"].reshape(B * T, C)
    row = a["cls"].astype(F32) + a["pos"].reshape(-1)[:C].astype(F32)
    assert row.dtype == F32
    want, written = f64(x), np.zeros((B * T, C), bool)
    want[::T], written[::T] = f64(row), True
    return want, np.zeros_like(want), written


def head_out(a):
    """-> (want, allow, decided: the pre-activation is negative beyond its error)"""
    C = a["C"]
    x, w, bias, md = f64(a["x"]).reshape(-1, C), f64(a["w"]), float(F32(a["bias"])), float(F32(a["max_depth"]))
    z = x @ w + bias
    e = (2 * C + 1) * U32 * (np.abs(x) @ np.abs(w) + abs(bias)) * SLACK
    want = np.maximum(z, 0.0) * md
    allow = (e * abs(md) + U32 * np.abs(want)) * SLACK
    decided = z < -e
    return want, np.where(decided, 0.0, allow), decided


def minmax_extremes(a):
    """-> (min, max) f32 [B], small [B]: fl32(max - min) < 1e-5f"""
    d = a["d"].reshape(a["B"], a["n"])
    assert d.dtype == F32 and np.isfinite(d).all(), "the contract is finite input"
    mn, mx = d.min(axis=1), d.max(axis=1)
    delta32 = mx - mn
    assert delta32.dtype == F32 and np.isfinite(delta32).all()
    return mn, mx, delta32 < F32(1e-5)


def minmax(a):
    """-> (want, allow, at_min) [B, n]"""
    d = f64(a["d"]).reshape(a["B"], a["n"])
    mn32, mx32, small = minmax_extremes(a)
    mn, mx = f64(mn32)[:, None], f64(mx32)[:, None]
    s = np.where(small[:, None], 1.0, 1.0 / np.where(small[:, None], 1.0, mx - mn))
    want = (d - mn) * s
    allow = np.where(small[:, None], U32 * np.abs(want), U32 * (3 * np.abs(want) + (np.abs(d) + np.abs(mn)) * s)) * SLACK
    at_min = d == mn  # (-0.0 == +0.0: both zeros of an image whose minimum is zero)
    return want, np.where(at_min, 0.0, allow), at_min


def f32_to_u8(src):
    v = np.fmin(np.fmax(np.asarray(src, F32), F32(0)), F32(1))
    prod = v * F32(255)
    assert prod.dtype == F32
    return prod.astype(np.uint8)  # truncation; every product lies in [0, 255]


def tvpre(a, hi=None):
    p, e = norm_div(a["rgb"].reshape(-1, 3), IMAGENET_MEAN, IMAGENET_INV)
    return residue_pixels(p, e, hi)


def half_axis(n_src, n_out):
    """float64 source coordinate of every output row (column), its cell, its weight, and the bound of the f32 coordinate's error"""
    f = np.arange(n_out) * ((n_src - 1) / (n_out - 1)) if n_out > 1 else np.zeros(1)
    i0 = np.minimum(np.floor(f).astype(np.int64), n_src - 1)
    return i0, np.minimum(i0 + 1, n_src - 1), f - i0, 2 * U32 * f


def bilinear_half(p, e):
    """p, e [B, H, W, 3] -> (value, f32 allowance) [B, H/2, W/2, 3]"""
    _, H, W, _ = p.shape
    y0, y1, ty, dfy = half_axis(H, H // 2)
    x0, x1, tx, dfx = half_axis(W, W // 2)
    ty, tx = ty[None, :, None, None], tx[None, None, :, None]

    def tap(t, ys, xs):
        return t[:, ys][:, :, xs]
    a, b, c, d = tap(p, y0, x0), tap(p, y0, x1), tap(p, y1, x0), tap(p, y1, x1)
    top, bot = a + (b - a) * tx, c + (d - c) * tx
    v = top + (bot - top) * ty
    big = np.max(np.abs([a, b, c, d]), axis=0)
    e_in = np.max([tap(e, y0, x0), tap(e, y0, x1), tap(e, y1, x0), tap(e, y1, x1)], axis=0)
    # the steepest slopes among source rows y0 - 1 .. y0 + 2 and columns x0 - 1 .. x0 + 2 (clamped: a repeated row adds a difference of zero)
    ys = np.clip(y0[:, None] + np.arange(-1, 3)[None, :], 0, H - 1)   # [OH, 4]
    xs = np.clip(x0[:, None] + np.arange(-1, 3)[None, :], 0, W - 1)   # [OW, 4]
    nb = p[:, ys][:, :, :, xs]                                        # [B, OH, 4, OW, 4, 3]
    ly = np.abs(np.diff(nb, axis=2)).max(axis=(2, 4))
    lx = np.abs(np.diff(nb, axis=4)).max(axis=(2, 4))
    e32 = e_in + 10 * U32 * big + dfy[None, :, None, None] * ly + dfx[None, None, :, None] * lx
    return v, e32 * SLACK


def bfhalf(a, hi=None):
    p, e = norm_mul(a["rgb"].reshape(a["B"], a["H"], a["W"], 3))
    v, e32 = bilinear_half(p, e)
    return residue_pixels(v.reshape(-1, 3), e32.reshape(-1, 3), hi)


def bfpatches(a):
    """-> (want, allow) [B h w, CP]"""
    B, h, w, gh, gw = (a[k] for k in ("B", "h", "w", "gh", "gw"))
    p, e = norm_mul(a["rgb"].reshape(B, gh * h, gw * w, 3))

    def chan(t):  # [B, gy, py, gx, px, c] -> [B, py, px, c, gy, gx]: channel gx + gw (gy + gh c)
        return t.reshape(B, gh, h, gw, w, 3).transpose(0, 2, 4, 5, 1, 3).reshape(B * h * w, 3 * gh * gw)
    return chan(p), chan(e + round16(np.abs(p) + e))


def sam_axis(n_src, n_dst):
    """the kernel's source coordinate of every output column (row) in float32 -> (first tap, second tap, weight of the second as float64)"""
    scale = F32(n_src) / F32(n_dst)
    s = np.maximum((np.arange(n_dst).astype(F32) + F32(0.5)) * scale - F32(0.5), F32(0))
    i0 = s.astype(np.int64)
    w = s - i0.astype(F32)
    assert s.dtype == F32 and w.dtype == F32 and i0.max() <= n_src - 1
    return i0, np.minimum(i0 + 1, n_src - 1), f64(w)


def sam_source(a):
    """the [sh, sw] plane the call reads, as float64"""
    sh, sw, sstride, step = a["sh"], a["sw"], a["sstride"], a["step"]
    idx = a["offset"] + (np.arange(sh)[:, None] * sstride + np.arange(sw)[None, :]) * step
    return f64(a["src"].reshape(-1)[idx])


def sam_values(a):
    """-> (value, allowance) [dh, dw] of the f32 result"""
    src = sam_source(a)
    x0, x1, wx = sam_axis(a["sw"], a["dw"])
    y0, y1, wy = sam_axis(a["sh"], a["dh"])
    v00, v01, v10, v11 = src[y0][:, x0], src[y0][:, x1], src[y1][:, x0], src[y1][:, x1]
    wx, wy = wx[None, :], wy[:, None]
    v = (1 - wy) * ((1 - wx) * v00 + wx * v01) + wy * ((1 - wx) * v10 + wx * v11)
    big = np.max(np.abs([v00, v01, v10, v11]), axis=0)
    return v, 6 * U32 * big * SLACK


def sam_undecided(a) -> int:
    """pixels of a u8 output whose float64 value lies within its allowance of the threshold"""
    v, e = sam_values(a)
    return int((np.abs(v) <= e).sum())


# ---- evaluate --------------------------------------------------------------------------------------------------------------------------------

def out_dtype(entry, a):
    if entry == "u8" or (entry == "sam" and a["out_u8"]):
        return np.uint8
    return np.float16 if entry in ("patches", "tvpre", "bfhalf", "bfpatches") else np.float32


def min_guard(entry, a) -> int:
    """one full block's worth of the kernel's stores behind the last element"""
    if entry in ("patches", "tvpre", "bfhalf", "bfpatches"):
        return BLOCK * 8
    if entry == "cls":
        return max(a["C"], 128)
    return BLOCK * 4


def initial_buffer(entry, a, size):
    """what the output buffer holds before the call; buffer_check.violations(got, ref, untouched=this) is the comparison"""
    dtype = out_dtype(entry, a)
    buf = np.full(size, CANARY_U8 if dtype == np.uint8 else CANARY, dtype)
    if entry == "cls":
        buf[:a["x"].size] = a["x"].reshape(-1)
    return buf


def _flat(want, allow, written, guard, fill):
    n = want.size
    full_w, full_a, full_m = np.full(n + guard, float(fill)), np.zeros(n + guard), np.zeros(n + guard, bool)
    full_w[:n], full_a[:n], full_m[:n] = want.reshape(-1), allow.reshape(-1), np.broadcast_to(written, want.shape).reshape(-1)
    return full_w, full_a, full_m  # (an element of the in-place entry that is not written expects its prior value)


def evaluate(entry: str, a, guard: int, got=None):
    """`got`: the buffer under test, for the entries with residue channels (their reference is the value minus the STORED hi)"""
    assert guard >= min_guard(entry, a)
    written = True
    if entry == "patches":
        want, allow = patches(a)
    elif entry == "pre32":
        want, allow = pre32(a)
    elif entry == "cls":
        want, allow, written = cls_rows(a)
    elif entry == "head_out":
        want, allow, _ = head_out(a)
    elif entry == "minmax":
        want, allow, _ = minmax(a)
    elif entry == "u8":
        want = f64(f32_to_u8(a["src"]))
        allow = np.zeros_like(want)
    elif entry in RESIDUE_ENTRIES:
        hi = None if got is None else np.asarray(got).reshape(-1)[:-guard].reshape(-1, 8)[:, :3]
        want, allow = (tvpre if entry == "tvpre" else bfhalf)(a, hi)
    elif entry == "bfpatches":
        want, allow = bfpatches(a)
    else:
        assert entry == "sam"
        want, allow = sam_values(a)
        if a["out_u8"]:
            want, allow = np.where(want > 0, 255.0, 0.0), np.zeros_like(want)
    return _flat(want, allow, written, guard, CANARY_U8 if out_dtype(entry, a) == np.uint8 else CANARY)


def zero_bit_elements(entry, a, size):
    """the elements of the flat output that must hold zero BITS (+0, not -0): the pad columns of the patches, channels 6..7 of a residue pixel,
    a head output whose pre-activation is negative beyond its error, the minimum of every normalised image"""
    out = np.zeros(size, bool)
    if entry == "patches":
        rows = a["B"] * (a["H"] // a["ps"]) * (a["W"] // a["ps"])
        m = np.zeros((rows, a["Kp"]), bool)
        m[:, a["ps"] * a["ps"] * 3:] = True
    elif entry in RESIDUE_ENTRIES:
        n = a["n"] if entry == "tvpre" else a["B"] * (a["H"] // 2) * (a["W"] // 2)
        m = np.zeros((n, 8), bool)
        m[:, 6:] = True
    elif entry == "head_out":
        m = head_out(a)[2]
    elif entry == "minmax":
        m = minmax(a)[2]
    else:
        return out
    out[:m.size] = m.reshape(-1)
    return out


# ---- the u8 twin of buffer_check: bytes, allowance 0 everywhere -------------------------------------------------------------------------------

def u8_violations(got, ref, untouched) -> dict:
    """-> dict(stray: bytes the call must leave alone that differ from `untouched`, first_stray, outside: written bytes that differ from the
    reference, worst: the first of them, ratio: 0.0 or inf, nonfinite: 0) -- buffer_check.violations' verdicts for a u8 buffer"""
    want, allow, written = ref
    assert got.dtype == np.uint8 and got.shape == want.shape == written.shape and not allow.any() and written.dtype == bool
    fill = np.broadcast_to(np.asarray(untouched, np.uint8), got.shape)
    stray = (got != fill) & ~written
    outside = (got.astype(np.float64) != want) & written
    return dict(stray=int(stray.sum()), first_stray=int(np.argmax(stray)), nonfinite=0, outside=int(outside.sum()), worst=int(np.argmax(outside)),
                ratio=float("inf") if outside.any() else 0.0)


def assert_u8_buffer(got, ref, what, untouched) -> dict:
    v = u8_violations(got, ref, untouched)
    assert v["stray"] == 0, f"{what}: {v['stray']} bytes written that the call must leave alone, the first at {v['first_stray']}"
    w = v["worst"]
    assert v["outside"] == 0, f"{what}: {v['outside']} of {got.size} bytes differ; the first at {w}: got {got[w]}, want {ref[0][w]:.0f}"
    return v

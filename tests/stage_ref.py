"""float64 references of the MI-GAN and YOLOv9t stage kernels -- csrc/kernels_migan.hip (vx_migan_dwconv_f16, plain and down kernel,
vx_migan_upsample_f16, vx_migan_torgb) and csrc/kernels_yolov9t.hip (vx_yolo_avgpool2_f16, vx_yolo_spp_f16, vx_yolo_upsample2_f16,
vx_yolo_decode) -- with a per-element allowance derived from the kernel's rounding steps, never from device output. Plain numpy, nothing from
the device side.

`evaluate(entry, args, guard, part=None)` -> (want, allow, written) over the WHOLE output buffer (flat: the buffer and `guard` elements behind
its last one) as the call leaves a buffer that started as `initial_buffer` gives it: filled with CANARY, except that vx_yolo_spp_f16's buffer
holds its input in channels [0, C) of every pixel (the call works in place and those must keep their bits). vx_yolo_decode has two dense
outputs, `part` = "boxes" and "scores"; its candidate list is compared exactly by `candidate_faults`.

Entries (`args` holds numpy arrays of the whole operands in the type the kernel reads; a FIR is f32 [4, 4, C]: tap row, tap column, channel):
  dw         vx_migan_dwconv_f16, down_fir NULL   x f16 [B, H, W, C], w f16 [3, 3, C], bias f32 [C] -> f16 [B, H, W, C]
  dw_down    vx_migan_dwconv_f16 with down_fir    the same, then the 4x4 FIR at stride 2, pad 1 -> f16 [B, H/2, W/2, C]
  up         vx_migan_upsample_f16                y f16 [B, h, w, C], fir, noise f32 [2h, 2w] | None, feat f16 | None -> f16 [B, 2h, 2w, C]
  torgb      vx_migan_torgb                       x f16 [B, H, W, C], w f32 [3, C], bias f32 [3], prev f32 [B, H/2, W/2, 3] | None, fir [4, 4, 3]
  avgpool2   vx_yolo_avgpool2_f16                 channels [c0, c0 + C) of x f16 [B, H, W, pix] -> f16 [B, H-1, W-1, C]
  spp        vx_yolo_spp_f16                      buf f16 [B, H, W, pix] in place: channels [C, 4C) = the 5, 9, 13 window maxima of [0, C)
  upsample2  vx_yolo_upsample2_f16                channels [c0, c0 + C) of x [B, h, w, x_pix] -> channels [o0, o0 + C) of y [B, 2h, 2w, y_pix]
  decode     vx_yolo_decode                       raw0..2 f16 [B, S/8 | S/16 | S/32 squared, 64 + nc] -> boxes f32 [B, A, 4], scores [B, A, nc]

The allowances (u16 = 2^-11, u32 = 2^-24, TINY16 = half the f16 subnormal step; SLACK = 1 + 2^-20 covers the products of two error terms):
  sums       n fma terms in f32 in any order (contracted or not), on f16 or f32 operands that are exact in f32, lie within (n + 1) u32 times
             (the sum of |terms| + |bias|): 9 terms for the depthwise, 16 for the down FIR, at most 4 for a polyphase upsample (+ 1 for the
             separate add of the noise, which enters the sum of magnitudes), C + 4 for torgb: (C + 5) u32 (|x| . |w| + |bias| + |prev| . |fir|).
  lrelu_agc  monotone with slope at most sqrt2: the incoming error passes through the slope (1 or 0.2), a negative value takes one f32
             rounding of 0.2f v and 0.2f's distance from 0.2, then everything is multiplied by the f32 gain 1.41421356f: the error times that
             gain, one f32 rounding of the product, and the constant's distance from sqrt(2) times the value.
  clamp      where |pre-activation| sqrt2 exceeds 256 by more than that allowance the result is exactly +-256: allowance 0, and it stays 0 through
             the rounding to f16 (256 is an f16 number) wherever no f32 add follows: every such output of the plain depthwise kernel and of
             the upsample without feat must be +-256 itself. Within the allowance of the edge either side is allowed: the clamp is
             1-Lipschitz, so the allowance of the unclamped value holds for the clamped one.
  f16        one rounding at the end: e + round16(|want| + e). The down kernel's intermediate stays f32 (LDS): its activation carries the f32
             allowance alone into the FIR, whose 16 terms add 17 u32 sum |act| |fir| and pass the activation's allowance through |fir|.
  upsample   the feat add comes after the activation, in f32 (one rounding of the sum), before the single f16 rounding.
  avgpool2   three f32 adds (3 u32 on the sum of magnitudes), an exact scale by 0.25, one f16 rounding.
  spp, upsample2   bit equality (`bit_faults`: the written elements' bits, so a zero keeps its sign), allowance 0: comparisons and copies. The clipped windows of radius 2, 4, 6 equal the chained 5x5 pools with
             -inf padding (tests/test_stage_ref_cpu.py pins them to yolov9t_ref.max_pool5 chained); the tables hold no -0.0 and no NaN in a spp
             input, so the maximum's bits are decided.
  decode     boxes: the float64 softmax expectation of yolov9t_ref.decode. With t_k = v_k - m (one rounding each: 16 subtractions) and
             e_k = expf(t_k), e_k carries the relative error r_k = u32 |t_k| (its argument) + EXP_ULPS 2^-23 (the device expf). The sum: 15
             adds, <= 16 u32 sum, plus sum r_k e_k. The weighted sum: 16 products by k (u32 each) and 16 adds: sum (r_k + u32) k e_k + 16 u32
             wsum. The division d = wsum / sum: E_wsum / sum + d E_sum / sum + u32 d. The anchor sum: u32 |anchor -+ d|. The stride product is
             exact (a power of two). scores: s = 1 / (1 + expf(-h)): -h is exact, e carries EXP_ULPS 2^-23 e, 1 + e one rounding, the division
             one: s^2 e EXP_ULPS 2^-23 + 2 u32 s; + 2^-126 where a device flushes an f32 subnormal. exp overflow (h = -65504) gives exactly 0
             and underflow exactly 1 in float64 too.
  EXP_ULPS   the device expf's own error in f32 ulps is the one number that is not derived. The ROCm installation ships no copy of the HIP math
             accuracy table, so it is 3, the bound OpenCL requires of exp, which the ROCm device library is built to. DESIGN.md records the largest error / allowance seen on exp-based elements.

The candidate list (`candidate_faults`): exact, no allowance. cand_count[b] = the number of STORED f32 scores of image b >= conf; the first
cand_count[b] entries of the region starting at b A nc are a permutation of those anchor nc + class indices; every cand_score is bit equal
to the dense score it names; everything behind the count and the guard behind the last region keeps the canary. `undecided` counts class
scores whose allowance interval (clipped to the sigmoid's range [0, 1]) straddles conf: the tables hold none, so the candidate set also equals
the float64 reference's."""
from __future__ import annotations

import numpy as np

import fir_ref
from block_ref import TINY16, U16, U32, round16  # noqa: F401

CANARY = -24000.0        # finite, exact in f16 and f32; no case writes a value within 1000 of it (tests/test_stage_ref_cpu.py)
CANARY_I32 = -1515870811  # 0xA5A5A5A5: no candidate index
SLACK = 1.0 + 2.0 ** -20
F32 = np.float32
EXP_ULPS = 3.0
ULP32 = 2.0 ** -23
TINY32 = 2.0 ** -126
BLOCK = 256
GAIN32 = float(F32(1.41421356))
SLOPE32 = float(F32(0.2))
SQRT2 = float(np.sqrt(2.0))
CLAMP = 256.0
ENTRIES = ("dw", "dw_down", "up", "torgb", "avgpool2", "spp", "upsample2", "decode")
FIR_ENTRIES = ("dw_down", "up", "torgb")
SCORE_CEILING, BOX_CEILING_PER_S = 1e-5, 1e-3  # what test_decode_dense_and_candidates_agree asserts


def f64(a):
    return np.asarray(a).astype(np.float64)


# ---- MI-GAN ------------------------------------------------------------------------------------------------------------------------------------

def agc(pre, e):
    """lrelu_agc of the float64 pre-activation with f32 allowance e -> (value, f32 allowance: 0 where the clamp decides, unclamped value)"""
    pre = f64(pre)
    neg = pre < 0
    t = np.where(neg, 0.2 * pre, pre)
    maybe_neg = pre < e
    e_t = e + np.where(maybe_neg, (U32 + abs(SLOPE32 / 0.2 - 1.0)) * 0.2 * np.abs(pre), 0.0)
    g = t * SQRT2
    e_g = (e_t * GAIN32 + (U32 + abs(GAIN32 / SQRT2 - 1.0)) * np.abs(g)) * SLACK
    decided = np.abs(g) - e_g > CLAMP
    return np.clip(g, -CLAMP, CLAMP), np.where(decided, 0.0, e_g), g


def to_f16(want, e, exact=False):
    """the allowance after the one rounding to f16; `exact`: the f32 value is decided and an f16 number (the clamp's +-256): nothing is allowed"""
    return np.where(exact, 0.0, e + round16(np.abs(want) + e))


def clamp_decided(e, g):
    """where agc()'s result is exactly +-256: the unclamped value lies beyond the clamp by more than its allowance"""
    return (e == 0) & (np.abs(g) > CLAMP)


def dw_pre(a):
    """the depthwise 3x3 + bias -> (pre-activation, its f32 allowance)"""
    x, w, bias = f64(a["x"]), f64(a["w"]), f64(a["bias"])
    pre = fir_ref.depthwise(x, w, bias, 1, 1)
    mag = fir_ref.depthwise(np.abs(x), np.abs(w), np.abs(bias), 1, 1)
    return pre, 10 * U32 * mag * SLACK


def dw_act(a):
    """-> (activation, f32 allowance, unclamped activation)"""
    return agc(*dw_pre(a))


def dw(a):
    v, e, g = dw_act(a)
    return v, to_f16(v, e, clamp_decided(e, g))


def dw_down(a, fir=None):
    v, e, _ = dw_act(a)
    f = f64(a["fir"] if fir is None else fir)
    want = fir_ref.depthwise(v, f, None, 2, 1)
    e32 = (fir_ref.depthwise(e, np.abs(f), None, 2, 1) + 17 * U32 * fir_ref.depthwise(np.abs(v), np.abs(f), None, 2, 1)) * SLACK
    return want, to_f16(want, e32)


def up_pre(a, fir=None):
    y, f = f64(a["y"]), f64(a["fir"] if fir is None else fir)
    nz = 0.0 if a["noise"] is None else f64(a["noise"])[None, :, :, None]
    raw = fir_ref.upfirdn2x_raw(y, f)
    mag = fir_ref.upfirdn2x_raw(np.abs(y), np.abs(f)) + np.abs(nz)
    return raw + nz, 6 * U32 * mag * SLACK


def up_act(a, fir=None):
    return agc(*up_pre(a, fir))


def up(a, fir=None):
    v, e, g = up_act(a, fir)
    exact = clamp_decided(e, g)
    if a["feat"] is not None:  # (an f32 add behind the clamp: its rounding and the f16 rounding of the sum are allowed again)
        v = v + f64(a["feat"])
        e = (e + U32 * np.abs(v)) * SLACK
        exact = False
    return v, to_f16(v, e, exact)


def torgb(a, fir=None):
    x, w, bias = f64(a["x"]), f64(a["w"]), f64(a["bias"])
    want, mag = x @ w.T + bias, np.abs(x) @ np.abs(w).T + np.abs(bias)
    if a["prev"] is not None:
        f = f64(a["fir"] if fir is None else fir)
        want = want + fir_ref.upfirdn2x_raw(f64(a["prev"]), f)
        mag = mag + fir_ref.upfirdn2x_raw(np.abs(f64(a["prev"])), np.abs(f))
    return want, (a["x"].shape[-1] + 5) * U32 * mag * SLACK


def clamp_share(entry, a) -> float:
    """the share of activations the clamp acts on in the reference (beyond the allowance)"""
    v, e, g = dw_act(a) if entry in ("dw", "dw_down") else up_act(a)
    return float(clamp_decided(e, g).mean())


def negative_share(entry, a) -> float:
    pre, e = dw_pre(a) if entry in ("dw", "dw_down") else up_pre(a)
    return float((pre < -e).mean())


def fir_variants(fir):
    """the three mistakes a symmetric filter hides: taps flipped, transposed, the parity taps 1 and 3 swapped (rows and columns)"""
    fir = np.asarray(fir)
    swap = [0, 3, 2, 1]
    return dict(flipped=fir[::-1, ::-1], transposed=fir.transpose(1, 0, 2), parity=fir[swap][:, swap])


# ---- YOLOv9t -----------------------------------------------------------------------------------------------------------------------------------

def avgpool2(a):
    x = f64(a["x"])[..., a["c0"]:a["c0"] + a["C"]]
    taps = (x[:, :-1, :-1], x[:, :-1, 1:], x[:, 1:, :-1], x[:, 1:, 1:])
    want = sum(taps) * 0.25
    e = 3 * U32 * sum(np.abs(t) for t in taps) * 0.25 * SLACK
    return want, to_f16(want, e)


def window_max(x, r, pad=-np.inf):
    """the maximum over the window of radius r clipped to the map: x [B, H, W, C] (`pad`: what lies outside; -inf never wins)"""
    B, H, W, C = x.shape
    p = np.full((B, H + 2 * r, W + 2 * r, C), pad)
    p[:, r:r + H, r:r + W] = x
    out = np.full(x.shape, -np.inf)
    for dy in range(2 * r + 1):
        for dx in range(2 * r + 1):
            out = np.maximum(out, p[:, dy:dy + H, dx:dx + W])
    return out


def spp(a):
    """-> (want, written) [B, H, W, pix]: the input in [0, C) (prior contents), the maxima in [C, 4C), the canary behind"""
    C = a["C"]
    buf = f64(a["buf"])
    want, written = np.full(buf.shape, CANARY), np.zeros(buf.shape, bool)
    x = buf[..., :C]
    want[..., :C] = x
    for i, r in enumerate((2, 4, 6)):
        want[..., (i + 1) * C:(i + 2) * C] = window_max(x, r)
    written[..., C:4 * C] = True
    return want, written


def upsample2(a):
    """-> (want, written) [B, 2h, 2w, y_pix]"""
    x = f64(a["x"])[..., a["c0"]:a["c0"] + a["C"]]
    B, h, w, _ = x.shape
    want, written = np.full((B, 2 * h, 2 * w, a["y_pix"]), CANARY), np.zeros((B, 2 * h, 2 * w, a["y_pix"]), bool)
    want[..., a["o0"]:a["o0"] + a["C"]] = x.repeat(2, axis=1).repeat(2, axis=2)
    written[..., a["o0"]:a["o0"] + a["C"]] = True
    return want, written


def grids(S):
    return S // 8, S // 16, S // 32


def n_anchors(S):
    return sum(g * g for g in grids(S))


def decode_boxes(a):
    """-> (boxes, allowance) [B, A, 4]"""
    boxes, allow = [], []
    for lv, r in enumerate(a["raws"]):
        B, g, _, ch = r.shape
        stride = 8.0 * 2 ** lv
        v = f64(r).reshape(B, g * g, ch)[..., :64].reshape(B, g * g, 4, 16)
        t = v - v.max(-1, keepdims=True)
        with np.errstate(under="ignore"):
            e = np.exp(t)
        k = np.arange(16.0)
        rel = U32 * np.abs(t) + EXP_ULPS * ULP32
        s, ws = e.sum(-1), (e * k).sum(-1)
        e_s = (rel * e).sum(-1) + 16 * U32 * s + 16 * TINY32
        e_ws = ((rel + U32) * k * e).sum(-1) + 16 * U32 * ws + 16 * 15 * TINY32
        d = ws / s
        e_d = e_ws / s + d * e_s / s + U32 * d
        gy, gx = np.meshgrid(np.arange(g), np.arange(g), indexing="ij")
        anc = np.stack([gx.ravel() + 0.5, gy.ravel() + 0.5, gx.ravel() + 0.5, gy.ravel() + 0.5], -1)[None]
        side = anc + d * np.array([-1.0, -1.0, 1.0, 1.0])
        boxes.append(side * stride)
        allow.append((e_d + U32 * np.abs(side)) * stride * SLACK)
    return np.concatenate(boxes, 1), np.concatenate(allow, 1)


def decode_scores(a):
    """-> (scores, allowance) [B, A, nc]"""
    h = np.concatenate([f64(r).reshape(r.shape[0], -1, r.shape[-1])[..., 64:] for r in a["raws"]], 1)
    with np.errstate(over="ignore", under="ignore"):
        e = np.exp(-h)
        s = 1.0 / (1.0 + e)
        se = np.where(np.isfinite(e), s * s * np.where(np.isfinite(e), e, 0.0), 0.0)
    allow = (se * EXP_ULPS * ULP32 + 2 * U32 * s) * SLACK + np.where(s > 0, TINY32, 0.0)
    return s, allow


def undecided(a) -> int:
    """class scores whose allowance interval, clipped to [0, 1], holds values on both sides of conf"""
    s, e = decode_scores(a)
    conf = float(F32(a["conf"]))
    return int(((np.maximum(s - e, 0.0) >= conf) != (np.minimum(s + e, 1.0) >= conf)).sum())


def reference_candidates(a):
    """per image the sorted anchor nc + class indices of the float64 scores >= conf"""
    s, _ = decode_scores(a)
    return [np.flatnonzero(s[b].ravel() >= float(F32(a["conf"]))) for b in range(s.shape[0])]


def candidate_faults(a, scores, count, idx, score, guard) -> list:
    """the exact checks of the candidate list against the STORED dense scores f32 [B, A, nc]; count i32 [B + guard], idx i32 and score f32
    [B A nc + guard] as the call left buffers that started at 0 (count, as the header requires) and the canaries -> what is wrong (empty: nothing)"""
    B, A, nc = scores.shape
    conf, out = F32(a["conf"]), []
    if (count[B:] != CANARY_I32).any():
        out.append("a store behind cand_count")
    taken = np.zeros(B * A * nc + guard, bool)
    bits = np.ascontiguousarray(scores).view(np.uint32).reshape(B, A * nc)
    for b in range(B):
        want = np.flatnonzero(scores[b].ravel() >= conf)
        n = int(count[b])
        if n != want.size:
            out.append(f"image {b}: count {n}, {want.size} stored scores pass")
        n = min(max(n, 0), A * nc)
        lo = b * A * nc
        mine = idx[lo:lo + n]
        if not np.array_equal(np.sort(mine), want):
            out.append(f"image {b}: the first {n} indices are not a permutation of the passing ones")
        ok = (mine >= 0) & (mine < A * nc)
        if (np.ascontiguousarray(score[lo:lo + n]).view(np.uint32)[ok] != bits[b][mine[ok]]).any():
            out.append(f"image {b}: a candidate score is not the bits of the dense score it names")
        taken[lo:lo + n] = True
    if (idx[~taken] != CANARY_I32).any() or (np.ascontiguousarray(score).view(np.uint32)[~taken] != F32(CANARY).view(np.uint32)).any():
        out.append(f"an entry behind a count or in the guard was written, the first at {int(np.argmax((idx != CANARY_I32) & ~taken))}")
    return out


def bit_faults(got, ref) -> int:
    """written elements of an allowance-0 f16 buffer whose bits are not the reference's (a -0.0 for a +0.0 is one)"""
    want, allow, written = ref
    assert got.dtype == np.float16 and not allow.any()
    return int((np.ascontiguousarray(got).view(np.uint16) != want.astype(np.float16).view(np.uint16))[written].sum())


# ---- evaluate ------------------------------------------------------------------------------------------------------------------------------------

def out_dtype(entry, part=None):
    return np.float32 if entry in ("torgb", "decode") else np.float16


def min_guard(entry) -> int:
    """one full block's worth of the kernel's stores behind the last element: 8 f16 per thread, 3 f32 (torgb), 4 | 8 f32 (decode)"""
    return BLOCK * 8


def initial_buffer(entry, a, size, part=None):
    buf = np.full(size, CANARY, out_dtype(entry, part))
    if entry == "spp":
        body = buf[:a["buf"].size].reshape(a["buf"].shape)
        body[..., :a["C"]] = a["buf"][..., :a["C"]]
    return buf


def _flat(want, allow, written, guard):
    n = want.size
    full_w, full_a, full_m = np.full(n + guard, CANARY), np.zeros(n + guard), np.zeros(n + guard, bool)
    full_w[:n], full_a[:n], full_m[:n] = want.reshape(-1), allow.reshape(-1), np.broadcast_to(written, want.shape).reshape(-1)
    return full_w, full_a, full_m


def evaluate(entry: str, a, guard: int, part=None):
    assert guard >= min_guard(entry)
    written = True
    if entry == "dw":
        want, allow = dw(a)
    elif entry == "dw_down":
        want, allow = dw_down(a)
    elif entry == "up":
        want, allow = up(a)
    elif entry == "torgb":
        want, allow = torgb(a)
    elif entry == "avgpool2":
        want, allow = avgpool2(a)
    elif entry == "spp":
        want, written = spp(a)
        allow = np.zeros_like(want)
    elif entry == "upsample2":
        want, written = upsample2(a)
        allow = np.zeros_like(want)
    else:
        assert entry == "decode" and part in ("boxes", "scores")
        want, allow = decode_boxes(a) if part == "boxes" else decode_scores(a)
    return _flat(want, allow, written, guard)

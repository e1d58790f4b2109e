"""float64 references of the Depth-Anything head's matrix-core kernels and derived per-element error allowances. Plain numpy, nothing from the
device side. What tests/dconv_ref.py already derives (round16, the accumulation term, the bilinear term, the HEAD epilogue term) is imported.

`evaluate(entry, args, guard)` -> (want, allow, written): flat arrays over the WHOLE output buffer -- the call's B images followed by `guard`
elements -- as the call leaves a zero-initialised one: the expected content (float64), the allowance of every element (float64) and which
elements the call writes (bool). An element the call must not write has allowance 0, so `|got - want| <= allowance` also catches a stray store.
The guard is at least one full tile row of the kernel (`min_guard`): where the out-of-map rows of the last image's bottom tiles would land.

entry "headconv" (vx_headconv_bil_f16 at cin 32, vx_headconv_wide_bil_f16 at cin 64 / 128); args:
  x f16 [B, hs, ws, cin] (flat or shaped; elements behind the B images are ignored: the call must not read them)
  wfrag f16 flat: [cin/32 slices][9 taps x 2 k-steps][64 lanes][8], lane (m = lane & 31, h = lane >> 5) of (slice s, tap, ks) holds
        W[m][tap][32 s + 16 ks + 8 h .. + 7] (the header's layout; `pack_frag` / `unpack_frag`)
  bias f32 [32], w3 f32 [32], b3, scale, B, H, W, hs, ws, cin
  out f32 [B, H, W] = scale * relu(sum_n relu(conv3x3(resize(x)) + bias)[n] * w3[n] + b3); the resize is bilinear, align_corners, source
  coordinate o / ((n_out - 1) / (n_src - 1)) clamped as the kernels' src_index does (dconv_ref.bilinear_table).
entry "rcu" (vx_rcu_fused_f16); args: x f16 [B, H, W, 64], w1, w2 f16 [9][64 n][64 c] and wp f16 [64 n][64 c] or None with the eight 16-byte
  groups of row n at position g ^ ((n >> 1) & 7) (`pack_rcu` / `unpack_rcu`), b1, b2, bp f32 [64] or None, res2 f16 like x or None, B, H, W
  out f16 [B, H, W, 64] = P(conv2(relu(conv1(relu(x)) + b1)) + b2 + x [+ res2]); the intermediate is zero outside the map (conv2's padding).
entry "bilinear" (vx_bilinear_ac_f16); args: x f16 [B, H, W, C], B, H, W, C, OH, OW; out f16 [B, OH, OW, C], the plain resize.

The allowances (u16 = 2^-11, u32 = 2^-24), from the arithmetic only, never from device output:
  headconv  interpolation: a halo value is lerp2(lerp2(a, b, fx), lerp2(c, d, fx), fy) on packed halves, lerp2(v, w, f) = f * w + (v - f * v).
            Whether the compiler contracts that into fused multiply-adds is its choice; the form with the most roundings the source text allows
            rounds f * w, f * v, v - f v and the sum: 4 per lerp2, and a value passes two lerp2 in a row: 8 roundings of magnitudes <= M =
            max(|a|, |b|, |c|, |d|) (in fact f M, f M, (1 - f) M and M per lerp2: <= 3 M, which pays for the second-order terms). The weights
            rounded to f16 and the f32 coordinate as dconv_ref words them: dconv_ref.bilinear_term(M, max(hs, ws), 8) per input value, pushed
            through |w|. Accumulation (9 cin + 8) u32 on |x| (*) |w| + |bias| (any order: the MFMA's, the K slices'), pushed through |w3|;
            (32 + 8) u32 on the dot product; all times |scale|; no f16 rounding on the way out (dconv_ref.head_epilogue). A ReLU whose argument
            lies below zero by more than its own bound is exactly 0 on the device as well: that channel carries no error on, and an output
            clipped that way has allowance 0 (the zero regions of the `negative` cases are compared exactly).
            The bound is linear in sum |x| |w| |w3|: it is sharp (about 1 % of an element) for data without cancellation -- the `positive`
            and `negative` kinds of the case table -- and loose for zero-mean data.
  rcu       conv1: (576 + 8) u32 on |relu x| (*) |w1| + |b1|, then one f16 rounding of the intermediate; that error pushed through |w2| next to
            conv2's own (576 + 8) u32 term; one f16 rounding of conv2 + b2 and one per f16 add (+ x, + res2); the projection pushes everything
            through |wp|, adds (64 + 8) u32 on |v| (*) |wp| + |bp| and one rounding. A rounding of a value that already carries an error e is
            within u16 (|v| + e) of it: every rounding step multiplies the carried error by (1 + u16).
  bilinear  NOT the packed-f16 form: four f32 weights ((1 - dx), (1 - dy) and a product: 3 roundings each), an f32 blend (a product and up to three
            adds per term): 8 u32 M; the coordinate term 12 u32 max(H, W) M as above; one f16 rounding of the result. An identity resize has
            weights 1, 0, 0, 0 exactly: allowance 0, the output bits are the input bits."""
from __future__ import annotations

import numpy as np

import dconv_ref as R
from dconv_ref import U16, U32, round16  # noqa: F401

HALO_ROUNDINGS = 8
TILE_H, TILE_W = 16, 32  # the head kernels' output tile


# ---- operand layouts -----------------------------------------------------------------------------------------------------------------------

def pack_frag(rows: np.ndarray, cin: int) -> np.ndarray:
    """conv kernel rows [32][Kp] with k = (ky, kx, c) -> the A fragments of the header"""
    w = np.asarray(rows)[:, :9 * cin].reshape(32, 9, cin // 32, 2, 2, 8)  # [m][tap][s][ks][h][q]
    return np.ascontiguousarray(w.transpose(2, 1, 3, 4, 0, 5)).astype(np.float16).reshape(-1)  # [s][tap][ks][h][m][q]: lane = 32 h + m


def unpack_frag(frag: np.ndarray, cin: int) -> np.ndarray:
    """the A fragments -> float64 [9 taps][cin][32 cout]"""
    t = np.asarray(frag).reshape(cin // 32, 9, 2, 2, 32, 8)  # [s][tap][ks][h][m][q]
    return t.transpose(1, 0, 2, 3, 5, 4).reshape(9, cin, 32).astype(np.float64)


def pack_rcu(w: np.ndarray) -> np.ndarray:
    """[64 n, taps, 64 c] -> f16 [taps][64 n][64 c], the 16-byte groups of row n at position g ^ ((n >> 1) & 7)"""
    t = np.asarray(w).astype(np.float16).transpose(1, 0, 2).reshape(-1, 64, 8, 8)
    out = np.empty_like(t)
    n = np.arange(64)
    for g in range(8):
        out[:, n, g ^ ((n >> 1) & 7)] = t[:, n, g]
    return np.ascontiguousarray(out).reshape(-1)


def unpack_rcu(flat: np.ndarray) -> np.ndarray:
    """-> float64 [taps][64 c][64 n]"""
    t = np.asarray(flat).reshape(-1, 64, 8, 8)
    out = np.empty_like(t)
    n = np.arange(64)
    for g in range(8):
        out[:, n, g] = t[:, n, g ^ ((n >> 1) & 7)]
    return out.reshape(-1, 64, 64).transpose(0, 2, 1).astype(np.float64)


def min_guard(entry: str, args, tile_h: int | None = None) -> int:
    """elements of one full tile row of the kernel behind the last image"""
    if entry == "headconv":
        return TILE_H * args["W"]
    if entry == "rcu":
        return (tile_h or args["H"]) * args["W"] * 64
    return args["OW"] * args["C"]


# ---- the three contracts -----------------------------------------------------------------------------------------------------------------

def resize(src: np.ndarray, H: int, W: int):
    """float64 [B, hs, ws, C] -> (the bilinear align_corners resize [B, H, W, C], M = the largest magnitude among each value's four sources)"""
    hs, ws = src.shape[1:3]
    y0, y1, fy = R.bilinear_table(H, hs)
    x0, x1, fx = R.bilinear_table(W, ws)
    fy, fx = fy[None, :, None, None], fx[None, None, :, None]
    a, b, c, d = src[:, y0][:, :, x0], src[:, y0][:, :, x1], src[:, y1][:, :, x0], src[:, y1][:, :, x1]
    out = (a * (1 - fx) + b * fx) * (1 - fy) + (c * (1 - fx) + d * fx) * fy
    return out, np.maximum(np.maximum(np.abs(a), np.abs(b)), np.maximum(np.abs(c), np.abs(d)))


def _source(args, shape):
    n = int(np.prod(shape))
    return np.asarray(args["x"]).reshape(-1)[:n].astype(np.float64).reshape(shape)


def headconv(args):
    """-> (want, allow) [B, H, W], and the reference's own intermediates (for range checks)"""
    B, H, W, hs, ws, cin = (args[k] for k in ("B", "H", "W", "hs", "ws", "cin"))
    w9 = unpack_frag(args["wfrag"], cin)
    bias, w3 = np.asarray(args["bias"], np.float64), np.asarray(args["w3"], np.float64)
    xin, big = resize(_source(args, (B, hs, ws, cin)), H, W)
    dx = R.bilinear_term(big, max(hs, ws), HALO_ROUNDINGS)
    z = R.conv3x3(xin, w9) + bias
    mag = R.conv3x3(np.abs(xin), np.abs(w9)) + np.abs(bias)
    e = R.conv3x3(dx, np.abs(w9))
    want, allow = R.head_epilogue(z, e, mag, 9 * cin, w3, float(args["b3"]), float(args["scale"]), exact_clip=True)
    return want, allow, dict(halo=xin, conv=z)


def _bias(args, key):
    return np.zeros(64) if args.get(key) is None else np.asarray(args[key], np.float64)


def _rounded(v, e):
    return e * (1 + U16) + round16(v)


def rcu(args):
    B, H, W = args["B"], args["H"], args["W"]
    x = _source(args, (B, H, W, 64))
    w1, w2 = unpack_rcu(args["w1"]), unpack_rcu(args["w2"])
    b1, b2 = _bias(args, "b1"), _bias(args, "b2")
    a = np.maximum(x, 0.0)
    z1 = R.conv3x3(a, w1) + b1
    e = R.accumulation_term(576, R.conv3x3(a, np.abs(w1)) + np.abs(b1))
    mid = np.maximum(z1, 0.0)
    e = _rounded(mid, e)  # the intermediate is f16
    z2 = R.conv3x3(mid, w2) + b2
    e = R.conv3x3(e, np.abs(w2)) + R.accumulation_term(576, R.conv3x3(mid, np.abs(w2)) + np.abs(b2))
    e = _rounded(z2, e)
    v = z2 + x
    e = _rounded(v, e)
    if args.get("res2") is not None:
        v = v + np.asarray(args["res2"]).reshape(-1)[:x.size].astype(np.float64).reshape(x.shape)
        e = _rounded(v, e)
    inter = dict(conv1=z1, conv2=z2, sum=v)
    if args.get("wp") is not None:
        wp, bp = unpack_rcu(args["wp"])[0], _bias(args, "bp")
        z = v @ wp + bp
        e = e @ np.abs(wp) + R.accumulation_term(64, np.abs(v) @ np.abs(wp) + np.abs(bp))
        e = _rounded(z, e)
        v = z
    return v, e, inter


def bilinear(args):
    B, H, W, C, OH, OW = (args[k] for k in ("B", "H", "W", "C", "OH", "OW"))
    want, big = resize(_source(args, (B, H, W, C)), OH, OW)
    if (OH, OW) == (H, W):
        return want, np.zeros_like(want), {}
    e = (8 * U32 + 12 * U32 * max(H, W)) * big
    return want, _rounded(want, e), {}


def evaluate(entry: str, args, guard: int):
    want, allow, _ = {"headconv": headconv, "rcu": rcu, "bilinear": bilinear}[entry](args)
    n = want.size
    full_w, full_a, written = np.zeros(n + guard), np.zeros(n + guard), np.zeros(n + guard, bool)
    full_w[:n], full_a[:n], written[:n] = want.reshape(-1), allow.reshape(-1), True
    return full_w, full_a, written

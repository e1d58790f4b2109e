"""float64 reference of vx_attention_relpos_f16 (csrc/kernels_attn_relpos.hip) and its per-element allowance. Plain numpy, nothing from the device side.

`args`: q, k, v f16 [B, T, H, 64] token-major (T = gw * gh tokens in row-major grid order), q NOT pre-scaled; rel_h f16 [2 gh - 1, 64], rel_w f16 [2 gw - 1, 64];
B, H, gw, gh, scale (the f32 the launcher is given). out = softmax(scale q k^T + bias) v with
  bias[(qy, qx), (ky, kx)] = q . rel_h[qy - ky + gh - 1] + q . rel_w[qx - kx + gw - 1]                       (transformers' get_decomposed_rel_pos),
pinned to SamVisionAttention by tests/test_relpos_attn_ref_cpu.py. The bias, from the f16 values of q and the tables, goes as `add` into the masked problem form
of tests/attn_ref.py (s = a q.k + b add in the exp2 domain, a = scale log2e, b = log2e), whose `solve` gives the output and the allowance of the masked
kernel's arithmetic: tile = 32, P in f16, the unrounded p summed into l, four roundings relative to |s| + |m|. The four are, here: the constant log2e and the
product fl(scale) fl(log2e) inside qs, the ONE fma acc * qs + bias, and the subtraction of the running maximum.

What `solve` does not know is how the kernel forms `add`. It grants (hd + 8) u32 b |add| -- errors relative to the bias itself -- but the kernel's bias is a sum
of two f32 MFMA sums of 64 exact f16 x f16 products each, whose error is relative to the sum of the products' magnitudes, and three more roundings:
  products      each part is within (64 - 1) u32 sum_d |q_d| |rel_d| of its exact value in any summation order:  63 u32 (|q| . |rel_h[j]| + |q| . |rel_w[i]|)
  log2e         each part is multiplied by the f32 constant log2e before it is stored (the constant's rounding, the product's): 2 u32 (|P_h| + |P_w|)
  store         in f32, the accumulator's own format: no rounding
  sum           RH + RW is one f32 add: u32 |P_h + P_w| <= u32 (|P_h| + |P_w|)
so  ds_bias = log2e (63 u32 (|q| . |rel_h[j]| + |q| . |rel_w[i]|) + 3 u32 (|P_h| + |P_w|)),  its maximum over the keys of a query; a score error ds moves out_d
by at most 2 ln2 ds A_d (attn_ref.py, `scores`), A_d = sum_j p_j |v_jd|. This term is added to solve's; the exponential's F16_TOL of the call's largest output
follows as in attn_ref._fill. Nothing here is fitted to device output."""
from __future__ import annotations

import numpy as np

from attn_ref import F16_TOL, round16, solve  # noqa: F401  (round16: the output rounding inside solve's allowance)

U32 = 2.0 ** -24
LOG2E = 1.4426950408889634
LN2 = 0.6931471805599453
HD = 64


def f64(a):
    return np.asarray(a, np.float64)


def rel_parts(q, rel_h, rel_w, gw, gh, absolute=False):
    """q [T, hd], rel_h [2 gh - 1, hd], rel_w [2 gw - 1, hd] -> (P_h, P_w) [T, T]: the two parts of the bias of every (query, key) pair; absolute: of |q|, |rel|"""
    if absolute:
        q, rel_h, rel_w = np.abs(q), np.abs(rel_h), np.abs(rel_w)
    t = np.arange(gw * gh)
    y, x = t // gw, t % gw
    ph = (q @ rel_h.T)[t[:, None], y[:, None] - y[None, :] + gh - 1]
    pw = (q @ rel_w.T)[t[:, None], x[:, None] - x[None, :] + gw - 1]
    return ph, pw


def problems(a, with_bias=True):
    B, H, gw, gh = a["B"], a["H"], a["gw"], a["gh"]
    T = gw * gh
    assert a["q"].shape == a["k"].shape == a["v"].shape == (B, T, H, HD) and a["rel_h"].shape == (2 * gh - 1, HD) and a["rel_w"].shape == (2 * gw - 1, HD)
    rel_h, rel_w = f64(a["rel_h"]), f64(a["rel_w"])
    for b in range(B):
        for h in range(H):
            q = f64(a["q"][b, :, h])
            ph, pw = rel_parts(q, rel_h, rel_w, gw, gh)
            yield dict(kind="masked", tile=32, a=float(np.float32(a["scale"])) * LOG2E, b=LOG2E, add=ph + pw if with_bias else None, q=q, k=f64(a["k"][b, :, h]),
                       v=f64(a["v"][b, :, h]), parts=(ph, pw), rows=slice(b * T, (b + 1) * T), cols=slice(h * HD, (h + 1) * HD))


def bias_allowance(p, a, w):
    """the term of the header: 2 ln2 max_keys(ds_bias) A_d, [T, hd]"""
    ah, aw = rel_parts(p["q"], f64(a["rel_h"]), f64(a["rel_w"]), a["gw"], a["gh"], absolute=True)
    ph, pw = p["parts"]
    ds = LOG2E * ((HD - 1) * U32 * (ah + aw) + 3 * U32 * (np.abs(ph) + np.abs(pw)))
    return 2 * LN2 * ds.max(-1, keepdims=True) * (w @ np.abs(p["v"]))


def evaluate_relpos(a, guard_rows=0, with_bias=True):
    """-> (want, allow, written) of the whole output buffer [B * T + guard_rows, H * 64] as the call leaves a zero-initialised one. with_bias False: the same
    attention without the bias (what a kernel that dropped it would return; the CPU test holds it against the allowance)."""
    shape = (a["B"] * a["gw"] * a["gh"] + guard_rows, a["H"] * HD)
    want, allow, written = np.zeros(shape), np.zeros(shape), np.zeros(shape, bool)
    for p in problems(a, with_bias):
        out, al, w = solve(p)
        r, c = p["rows"], p["cols"]
        want[r, c], allow[r, c], written[r, c] = out, al + bias_allowance(p, a, w), True
    allow[written] += F16_TOL * np.abs(want[written]).max()  # the exponential: attn_ref.py's header
    return want, allow, written


# (gw, gh, heads, B): a single token; gw != gh with head and batch strides, and its transpose; two query tiles in one block, the second ragged (T = 49: the
# only case on the two-wave kernel); SAM's window (T = 196 is no tile multiple, key tiles straddle rows); a row wider than half a tile; the row-aligned form
# with the fewest rows; the global shape
CASES = [(1, 1, 1, 1), (3, 5, 2, 2), (5, 3, 2, 2), (7, 7, 2, 1), (14, 14, 2, 3), (20, 7, 1, 1), (64, 2, 1, 1), (64, 64, 1, 1)]


def operands(case, seed=0):
    """seeded standard normal q, k, v as f16; table entries of standard deviation 0.25, so each part of the bias has one of about 2"""
    gw, gh, H, B = case
    rng = np.random.default_rng(seed)
    q, k, v = (rng.standard_normal((B, gw * gh, H, HD)).astype(np.float16) for _ in range(3))
    rel_h = (rng.standard_normal((2 * gh - 1, HD)) * 0.25).astype(np.float16)
    rel_w = (rng.standard_normal((2 * gw - 1, HD)) * 0.25).astype(np.float16)
    return dict(q=q, k=k, v=v, rel_h=rel_h, rel_w=rel_w, B=B, H=H, gw=gw, gh=gh, scale=np.float32(0.125))

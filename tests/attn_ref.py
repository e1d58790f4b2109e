"""float64 references of the five attention entry points and a derived per-element error allowance. Plain numpy, nothing from the device side.

One `evaluate_*(args, guard_rows)` per entry point. `args` holds the launcher's own arguments, pointers replaced by numpy arrays that hold the
WHOLE buffer behind the pointer, with the f16 values the kernel reads:
  vx_attention_f16          q, k, v f16 [B, H, T, 64], q already multiplied by scale * log2(e);  B, H, T
  vx_attention_masked_f16   q, k, v f16 [B, H, T, head_dim], q scaled likewise; mask f16 / f32 [Bm, Hm, T, T];  B, H, T, head_dim, Hm, Bm, mask_is_f32
  vx_window_attention_*     qkv f16 [n_windows * N, heads, 3, 32]; bias [heads, N, N]: the f16 values of the table, -inf allowed; mask None or
                            [nwx * nwy, N, N] of 0 / -inf: the class masks, window w of the call reads mask[w % (nwx * nwy)];  n_windows, N, heads, nwx, nwy
  vx_small_attention_f16    q f16 [Nq, heads * hd], k, v f16 [Nk, heads * hd];  Nq, Nk, heads, hd
  vx_attention_cross_f16    q f16 [B, Tq, H, head_dim], k, v f16 [B, Tk, H, head_dim], token-major, q NOT pre-scaled;  B, H, Tq, Tk, head_dim, scale (the f32
                            the launcher is given). Problem (b, h) owns rows b * Tq .. and columns h * head_dim .. of the [B * Tq + guard, H * head_dim] buffer.
Each returns `want, allow, written` for the whole row-major output buffer [rows + guard_rows, heads * head_dim] as the call leaves a
zero-initialised buffer. The guard rows sit behind the last row the call owns; `allow` is 0 wherever the call must not write, so the one
comparison |got - want| <= allow also finds stray stores. A query whose mask is -inf on every key is unspecified by contract: `evaluate` refuses it.

All five are softmax2(s) v with s, in the exp2 domain, = a * (q . k) + b * add  (a, b = 1, 0 | 1, log2e | log2e / sqrt(32), log2e | log2e / sqrt(hd), 0 |
scale * log2e, 0; add = the mask, or bias + class mask). p = the softmax weights of a query, l their sum before the division, A_d = sum_j p_j |v_jd|, out_d = sum_j p_j v_jd,
u16 = 2^-11, u32 = 2^-24. The allowance of out_d is the sum of:
  scores        an f32 MFMA (or fma chain) sum of hd exact f16 x f16 products is within (hd - 1) u32 of the exact sum times sum_d |q_d| |k_d| in ANY
                order; the scale, the mask / bias fma, the constant log2e and the subtraction of the reference point m round a few more times, each
                relative to a value of at most |s| + |m|:  ds = (hd + 8) u32 (a sum|q||k| + b |add|) + 4 u32 (|s| + |m|), its maximum taken over the keys
                that can reach the output at all (s - m > -150: exp2 of less is 0 in f32). A score error ds scales p_j by 2^ds, so out_d = sum p_j v_jd / sum p_j
                moves by at most ln2 ds sum_j p_j |v_jd - out_d| <= 2 ln2 ds A_d.
  exponential   v_exp_f32 (and __expf, which is v_exp_f32 of the argument times log2e -- that product's rounding is one of the four above) has no
                accuracy bound in the guides or in any ISA text shipped with the toolchain, so, as for GELU in tests/gemm_ref.py, the project's
                F16_TOL = 4e-3 of the largest reference magnitude of the call. This is the largest term by far; the others are kept because they
                are what remains once the instruction's accuracy is pinned.
  P in f16      (MFMA kernels) every P is rounded to f16 before the PV product: the numerator moves by u16 A_d. The masked and window kernels sum the
                unrounded p into l, which is another u16 A_d through the denominator; vx_attention_f16 sums the rounded P, so numerator and denominator see
                the same factors (1 + e_j) and out_d moves by u16 sum p_j |v_jd - out_d| <= 2 u16 A_d: 2 u16 A_d either way. A P below 2^-14 is an f16
                subnormal, absolute error 2^-25 in the units of the reference point it was computed against: T 2^-25 max_j |v_jd| over l. The reference point
                of the masked and window kernels is the running maximum; that of vx_attention_f16 lags, but it is only ever set to the row maximum of a tile
                (first tile, or a full-path tile that raised it), so it is a score the row really has, never above the row's largest: the key that set it
                has P = 1, every later rescale multiplies l and that P alike and is followed by a new P = 1, so l >= 1 in the reference point's units at
                every moment and the subnormal term needs no division.
  row sum       (vx_attention_f16, VISP_ATTN_RS = 1) l's tile sums come from four levels of packed-f16 adds of positive values: relative error at most
                (1 + u16)^4 - 1, so 4 u16 |out_d| (plus second order, paid by the spare units of the next term).
  accumulation  O and l are f32 sums of T terms in n_tiles groups, each group followed by at most one rescale:  (T + n_tiles + 8) u32 A_d for O and the same
                times |out_d| <= A_d for l:  2 (T + n_tiles + 8) u32 A_d. vx_small_attention_f16 sums in a fixed order with n_tiles = 0; any-order bounds hold.
  output        max(u16 |out_d|, 2^-25) for the one rounding to f16; o * (1 / l) rounds twice in f32 (in the 8 spare units).

vx_attention_cross_f16 is the masked kernel's arithmetic (tile = 32, P in f16 and its subnormal term, the unrounded p summed into l: 2 u16 A_d and T_k 2^-25
max|v_d|, accumulation with n_tiles = ceil(T_k / 32)) with these differences, none of them fitted to what the device returns:
  scores        the kernel multiplies the f32 MFMA sum by the f32 qs = fl(fl(scale) fl(log2e)). Where the masked kernel has one fma (mask * log2e + acc) there
                are three roundings relative to |s| here (the constant log2e, the product that makes qs, the product acc * qs) and the subtraction of the
                reference point: one more than the four the header counts, so 5 u32 (|s| + |m|) in ds.
  key split     (T_q <= 32 and T_k >= 256: parts of 128 keys) block (bh, part i) leaves its unrounded f32 triple (m_i, l_i, O_i), the masked kernel's sums over
                its own <= 128 keys with m_i the part's largest score as the reference point: the terms above hold per part, and a sum over the parts of
                per-part bounds is at most the bound over all T_k keys (the subnormal term: a P of part i is off by 2^-25 in the units of a running maximum
                <= m_i <= m, and the rescales that follow only shrink it; in the units of m the key that holds m has P = 1, so l >= 1 up to rounding as before).
                The combine takes m = max m_i exactly and then, per part in part order,
                  w_i = exp2(m_i - m)   one subtraction, rounded relative to |m_i| + |m|: every p of part i is scaled by 2^(u32 (|m_i| + |m|)), which is a
                                        score error of that size on the keys of the part. m_i is the score of a key of the part; a part all of whose keys
                                        are dead (s - m <= -150) has w_i = 0 in f32 either way. One more unit: 6 u32 (|s| + |m|) in ds for a split. The
                                        accuracy of the exp2 itself is what the F16_TOL term stands for, as it is for every p.
                  l   = fma(l_i, w_i, l)     a chain of `parts` fma over positive terms: relative error at most parts u32 of the sum
                  acc = fma(O_id, w_i, acc)  the same chain over terms of either sign: at most parts u32 sum_i |O_id| w_i <= parts u32 l A_d
                so the division moves by parts u32 A_d through acc and parts u32 |out_d| <= parts u32 A_d through l:  2 parts u32 A_d on top of the
                accumulation term; acc * (1 / l) rounds twice in f32, in the 8 spare units as before."""
from __future__ import annotations

import numpy as np

U16, U32, TINY16 = 2.0 ** -11, 2.0 ** -24, 2.0 ** -25
F16_TOL = 4e-3  # tests/test_gpu_kernels.py
LOG2E = 1.4426950408889634
LN2 = 0.6931471805599453
DEAD = -150.0   # exp2 of less is 0 in f32, subnormals included


def f64(a):
    return np.asarray(a, np.float64)


def round16(x):
    """the allowance of one rounding of x to f16"""
    return np.maximum(U16 * np.abs(x), TINY16)


def scores2(p):
    """exp2-domain scores [Tq, Tk] of one problem (see `problems`), float64; -inf where `add` is"""
    s = p["a"] * (p["q"] @ p["k"].T)
    return s if p["add"] is None else s + p["b"] * p["add"]


def softmax2(s):
    m = s.max(-1, keepdims=True)
    assert np.isfinite(m).all(), "a query is masked on every key: unspecified by contract"
    w = np.exp2(s - m)
    return w / w.sum(-1, keepdims=True), m


def solve(p):
    """one (batch, head) / (window, head) problem -> out [Tq, hd], its allowance WITHOUT the exponential term, the weights [Tq, Tk]"""
    q, k, v = p["q"], p["k"], p["v"]
    hd, Tk = q.shape[1], k.shape[0]
    s = scores2(p)
    w, m = softmax2(s)
    out, A = w @ v, w @ np.abs(v)
    mag = p["a"] * (np.abs(q) @ np.abs(k).T)
    live = s - m > DEAD
    with np.errstate(invalid="ignore"):
        if p["add"] is not None:
            mag = mag + p["b"] * np.abs(np.where(live, p["add"], 0.0))
        n_round = 4 if p["kind"] != "cross" else (5 if p["parts"] == 1 else 6)   # the docstring: the cross kernel's qs product and its combine
        ds = np.where(live, (hd + 8) * U32 * mag + n_round * U32 * (np.abs(np.where(live, s, 0.0)) + np.abs(m)), 0.0)
        # a key below the cut stays below it: its score error is far smaller than its distance to the cut
        dead_err = np.where(live, 0.0, (hd + 8) * U32 * np.abs(np.where(np.isfinite(s), s, 0.0)))
        assert (np.where(live, -np.inf, s - m + dead_err) < DEAD + 20).all()
    allow = 2 * LN2 * ds.max(-1, keepdims=True) * A
    n_tiles = -(-Tk // p["tile"]) if p["tile"] else 0
    allow = allow + 2 * (Tk + n_tiles + 8) * U32 * A + round16(out)
    if p["tile"]:  # the MFMA kernels: P in f16
        allow = allow + 2 * U16 * A + Tk * TINY16 * np.abs(v).max(0)
    if p["kind"] == "dense":
        allow = allow + 4 * U16 * np.abs(out)
    if p["kind"] == "cross" and p["parts"] > 1:   # the combine's two fma chains
        allow = allow + 2 * p["parts"] * U32 * A
    return out, allow, w


def _buffer(rows, cols, guard_rows):
    shape = (rows + guard_rows, cols)
    return np.zeros(shape), np.zeros(shape), np.zeros(shape, bool)


def _fill(probs, rows, cols, guard_rows):
    want, allow, written = _buffer(rows, cols, guard_rows)
    for p in probs:
        out, al, _ = solve(p)
        r, c = p["rows"], p["cols"]
        want[r, c], allow[r, c], written[r, c] = out, al, True
    allow[written] += F16_TOL * np.abs(want[written]).max()  # the exponential: see the header
    return want, allow, written


# ---- the (rows, columns) problems of each entry point: what the reference, the emulations and the sensitivity condition all walk ---------------

def problems_attention(a):
    B, H, T = a["B"], a["H"], a["T"]
    assert a["q"].shape == a["k"].shape == a["v"].shape == (B, H, T, 64)
    for b in range(B):
        for h in range(H):
            yield dict(kind="dense", tile=64, a=1.0, b=0.0, add=None, q=f64(a["q"][b, h]), k=f64(a["k"][b, h]), v=f64(a["v"][b, h]),
                       rows=slice(b * T, (b + 1) * T), cols=slice(h * 64, (h + 1) * 64), b_idx=b, h_idx=h)


def problems_masked(a):
    B, H, T, hd, Hm, Bm = a["B"], a["H"], a["T"], a["head_dim"], a["Hm"], a["Bm"]
    assert a["q"].shape == a["k"].shape == a["v"].shape == (B, H, T, hd) and a["mask"].shape == (Bm, Hm, T, T)
    assert a["mask"].dtype == (np.float32 if a["mask_is_f32"] else np.float16)
    for b in range(B):
        for h in range(H):
            yield dict(kind="masked", tile=32, a=1.0, b=LOG2E, add=f64(a["mask"][b % Bm, 0 if Hm == 1 else h]), q=f64(a["q"][b, h]), k=f64(a["k"][b, h]),
                       v=f64(a["v"][b, h]), rows=slice(b * T, (b + 1) * T), cols=slice(h * hd, (h + 1) * hd), b_idx=b, h_idx=h)


def problems_window(a):
    n_win, N, heads, nwx, nwy = a["n_windows"], a["N"], a["heads"], a["nwx"], a["nwy"]
    qkv = a["qkv"]
    assert qkv.shape == (n_win * N, heads, 3, 32) and a["bias"].shape == (heads, N, N)
    assert (a["mask"] is None) == (nwx == 0) and (nwx == 0 or a["mask"].shape == (nwx * nwy, N, N))
    for w in range(n_win):
        for h in range(heads):
            add = f64(a["bias"][h]) if nwx == 0 else f64(a["bias"][h]) + f64(a["mask"][w % (nwx * nwy)])
            r = slice(w * N, (w + 1) * N)
            yield dict(kind="window", tile=32, a=LOG2E / np.sqrt(32.0), b=LOG2E, add=add, q=f64(qkv[r, h, 0]), k=f64(qkv[r, h, 1]), v=f64(qkv[r, h, 2]),
                       rows=r, cols=slice(h * 32, (h + 1) * 32), b_idx=w, h_idx=h)


def problems_small(a):
    Nq, Nk, heads, hd = a["Nq"], a["Nk"], a["heads"], a["hd"]
    assert a["q"].shape == (Nq, heads * hd) and a["k"].shape == a["v"].shape == (Nk, heads * hd)
    for h in range(heads):
        c = slice(h * hd, (h + 1) * hd)
        yield dict(kind="small", tile=0, a=LOG2E / np.sqrt(float(hd)), b=0.0, add=None, q=f64(a["q"][:, c]), k=f64(a["k"][:, c]), v=f64(a["v"][:, c]),
                   rows=slice(0, Nq), cols=c, b_idx=0, h_idx=h)


def cross_parts(Tq, Tk):
    """the launcher's rule, restated: at most one query block and at least 256 keys split the keys into parts of 128"""
    return -(-Tk // 128) if Tq <= 32 and Tk >= 256 else 1


def problems_cross(a):
    B, H, Tq, Tk, hd = a["B"], a["H"], a["Tq"], a["Tk"], a["head_dim"]
    assert a["q"].shape == (B, Tq, H, hd) and a["k"].shape == a["v"].shape == (B, Tk, H, hd)
    scale = np.float32(a["scale"])
    for b in range(B):
        for h in range(H):
            yield dict(kind="cross", tile=32, a=float(scale) * LOG2E, b=0.0, add=None, q=f64(a["q"][b, :, h]), k=f64(a["k"][b, :, h]), v=f64(a["v"][b, :, h]),
                       parts=cross_parts(Tq, Tk), qs=scale * np.float32(LOG2E), rows=slice(b * Tq, (b + 1) * Tq), cols=slice(h * hd, (h + 1) * hd), b_idx=b, h_idx=h)


PROBLEMS = {"attention": problems_attention, "masked": problems_masked, "window": problems_window, "small": problems_small, "cross": problems_cross}


def out_shape(entry, a):
    """(rows the call owns, columns) of the output buffer"""
    if entry == "attention":
        return a["B"] * a["T"], a["H"] * 64
    if entry == "masked":
        return a["B"] * a["T"], a["H"] * a["head_dim"]
    if entry == "window":
        return a["n_windows"] * a["N"], a["heads"] * 32
    if entry == "cross":
        return a["B"] * a["Tq"], a["H"] * a["head_dim"]
    return a["Nq"], a["heads"] * a["hd"]


def evaluate(entry, a, guard_rows=0):
    """-> (want, allow, written) of the whole output buffer [rows + guard_rows, columns] (float64, float64, bool)"""
    rows, cols = out_shape(entry, a)
    return _fill(PROBLEMS[entry](a), rows, cols, guard_rows)


def evaluate_attention(a, guard_rows=0):
    return evaluate("attention", a, guard_rows)


def evaluate_masked(a, guard_rows=0):
    return evaluate("masked", a, guard_rows)


def evaluate_window(a, guard_rows=0):
    return evaluate("window", a, guard_rows)


def evaluate_small(a, guard_rows=0):
    return evaluate("small", a, guard_rows)


def evaluate_cross(a, guard_rows=0):
    return evaluate("cross", a, guard_rows)

"""float64 reference of the token-stationary DINOv2 block kernel (vx_dino_block16_f16, csrc/kernels_block16.hip) and a derived per-element
error allowance. Plain numpy, nothing from the device side.

`evaluate(args, guard_rows, x_out=None)` -> {buffer: (want, allow, written)} for every buffer the call can touch -- x, cap_x1, feat, q, k, v -- as the call
leaves it, guards included: the expected content (float64), the allowance of every element (float64) and which elements the call writes (bool).
An element the call must not write has allowance 0, so `|got - want| <= allow` also catches a stray store. x keeps its INPUT in the guard rows,
every other buffer starts zeroed. The row-major buffers (x, cap_x1, feat: [M + guard_rows, 384]) carry `guard_rows` rows behind row M - 1
(128 = one workgroup's worth: where the dead rows of the last workgroup would land), q / k / v ([M / T + 1, 6, T, 64]) one whole extra image.

args (the launcher's own, numpy arrays for the whole buffers):
  x f32 [M + guard_rows, 384]; att f16 [M, 384] or None (no MLP half); wo, w1, w2, wqkv: the UNPACKED f16 weights [384][384], [1536][384],
  [384][1536], [1152][384] with LayerScale folded into wo / w2 (what vx_dino_block16_pack_mlp / _qkv take); vec_mlp, vec_qkv, vec_tap: the three
  f32 vectors of the header; M, T, H, q_scale, eps; feat, q, cap: whether the call is given feat, q / k / v, cap_x1;
  fc2_random_signs (default True): see the GELU term below.

The contract (dino.cpp:48-90 with the device's rounding points), all in float64:
  x1 = x + bo' + att Wo'^T                               (cap_x1)
  x2 = x1 + b2' + f16(gelu(f16(LN2(x1)) W1^T + b1)) W2'^T   (x)
  feat = LN_final(x2);  q | k | v = f16(LN1(x2)) Wqkv^T + bqkv, q times q_scale, head-major [B, 6, T, 64]
LayerNorm uses the biased variance with eps inside the square root; GELU is the tanh form. The LayerNorm rows and the activated hidden values
are rounded to f16 exactly where the device rounds them: they are MFMA operands.

The allowance (u16 = 2^-11, u32 = 2^-24), from the arithmetic only, never from device output. A worst-case interval sum through the three
chained products (K = 384, 1536, 384) is as large as the MLP branch itself and checks nothing, so it is built from these parts:

  sums      an f32 sum of K products in ANY order (the MFMA's, the k-blocks', the bias first or last): (K + 8) u32 (|A| |W|^T + |bias| +
            |accumulator input|). K counts the nonzero weights of the output row: exact zeros add nothing, which keeps the structured-weight
            probes sharp. The residual stream is the accumulator input of the out-projection and of fc2; its allowance is carried along.
  roundings one max(u16 |v|, 2^-25) per rounding to f16 on the way out (feat, q, k, v); q's f32 multiply by q_scale one u32 |v|.
  LayerNorm as the kernel writes it, x (rstd g) + (b - mean rstd g) in f32. With e_x the allowance the row arrives with:
              mean:     (D + 8) u32 mean|x| + mean(e_x)                                     =: e_mean;  e_d = e_x + e_mean per element
              variance: (D + 8) u32 var + 2 mean(|x - mean| e_d) + mean(e_d^2)              =: e_var;   t = e_var / (var + eps)
              rstd:     relative RSQ_REL + t / 2 + t^2   (|(1 + t)^-1/2 - 1| <= t / 2 + t^2 up to t = 0.6)
              value:    |rstd g| e_d + |x - mean| |rstd g| rel(rstd) + 4 u32 (|x rstd g| + |mean rstd g| + |b|)
            The last term is the two fused multiply-adds and the product rstd g on the magnitudes they really see: it grows for rows whose
            mean dwarfs their spread, as the e_mean term does.
            ASSUMPTION: v_rsq_f32 has no accuracy statement in the guides this project works from. Its relative error is assumed below
            RSQ_REL = u16 / 2 = 2^-12 -- thousands of f32 ulps of slack, and still below the f16 rounding that follows.
  flips     the reference rounds a LayerNorm value v to f16; the device rounds v + d, |d| <= e (the stage's own allowance above). Rounding is
            monotone, so the device's f16 lies in [f16(v - e), f16(v + e)]: the deviation dev = max(f16(v + e) - f16(v), f16(v) - f16(v - e))
            is 0 unless v lies within e of a rounding midpoint. Only those elements carry a deviation (one ulp, more where e exceeds an ulp)
            into the next product, weighted by |W|: dev |W|^T is part of the allowance of q, k, v and of the pre-activation z.
            With the worst-case (K + 8) u32 sums and RSQ_REL above, e is a good fraction of an f16 ulp, so on ordinary rows most LN2 elements
            CAN flip, and pushing dev |W1|^T through 1.13 and |W2'| as well (two worst cases in a row) came to three quarters of the MLP
            branch. The flips therefore go through the MLP linearised, still worst-case over their signs: per row m,
                sum_k |W2' diag(gelu'(z_m)) W1|[n, k] dev[m, k]  +  |W2'| (max|gelu''| / 2) allow_z^2
            (`flips_through_mlp`; |gelu''| <= 0.8, taken as 1; allow_z is the full allowance on z). The products inside the absolute value
            cancel as the kernel's do, which is what a worst case on each factor throws away: some 70 times tighter, and rigorous.
  GELU      hidden units 32 .. 1503 run `gelu_side` on packed f16: convert, clamp at -65504, x x, packed fma with the f16 constants, times x,
            exp2, + 1, rcp, times x, every result an f16. `gelu_f16_sequence` emulates that with numpy float16 (exp2 and rcp correctly
            rounded) and `gelu_envelope()` takes its largest error against the float64 GELU over every finite f16 input: GELU_ENV_FIGURE =
            2.08 u16 max(|z|, 1), at z = 2.22 (recomputed by tests/test_block_ref_cpu.py, which pins the figure written here). The per-unit
            allowance is that envelope TIMES 2: the device's v_exp_f16 / v_rcp_f16 are approximations of undocumented accuracy where the
            emulation's are correctly rounded, and a margin equal to the error of the whole rest of the sequence is generous for two
            instructions (about 4 f16 ulps in all). The envelope is over f16 INPUTS, so the conversion of the f32 pre-activation adds one
            rounding of z through the GELU's Lipschitz bound (< 1.13, as in gemm_ref.py); fc1's own sum term enters the same way, and the
            reference's own rounding of h to f16 is added. Units 0 .. 31 and 1504 .. 1535 run the f32 `gelu_block`, whose arithmetic is
            strictly finer: same allowance, their ratio reported on its own.
  GELU through fc2   a worst-case |W2'| allow_h is again useless. The dense cases draw W2' with independent random signs, and allow_h (envelope,
            conversion, 1.13 times fc1's sum term, the reference's rounding of h) bounds errors that are decided upstream of W2': the term is
            carried as 6 sqrt((W2'^2) allow_h^2), six sigma of a sum whose terms have independent signs. With at most about 2e7 compared
            elements in the whole matrix that expects well under one false failure. THIS TERM IS PROBABILISTIC AND RESTS ON THE TEST'S CHOICE
            OF WEIGHTS; cases with structured W2' (the probes) pass fc2_random_signs = False and get the worst case |W2'| allow_h, which for
            a one-hot row is the GELU allowance alone. Every other term stays worst-case.
  behind the MLP   feat, q, k, v are functions of the residual stream the kernel has just written (its accumulators ARE the stored x). With
            `x_out` (the x buffer as the device left it, itself compared against the allowance above) evaluate() returns feat, q, k, v of THAT
            stream, with their own stage's allowance only. Without it the allowance of x is carried into them through the LayerNorm terms,
            where the GELU's few f16 ulps are divided by a small row's spread and allow ten per cent and more.
First order throughout: an allowance carried into the next stage is not compounded with that stage's own relative terms (products of two
terms of 1e-4 and less)."""
from __future__ import annotations

import numpy as np

U16, U32, TINY16 = 2.0 ** -11, 2.0 ** -24, 2.0 ** -25
D, HID, HEADS = 384, 1536, 6
ROW_GUARD = 128          # guard rows of the row-major buffers: one workgroup
RSQ_REL = U16 / 2        # assumed relative accuracy of v_rsq_f32 (see above)
GELU_LIPSCHITZ = 1.13
GELU_CURVATURE = 1.0     # |gelu''| <= 0.8 (both checked on a grid by tests/test_block_ref_cpu.py)
GELU_MARGIN = 2.0      # envelope x 2: the device's exp2 / rcp are approximations
GELU_ENV_FIGURE = 2.08   # the envelope as a multiple of u16 max(|z|, 1), as written above; gelu_envelope() is what evaluate() uses
SIGMAS = 6.0
F32_UNITS = np.r_[0:32, HID - 32:HID]  # hidden blocks 0 and 47: gelu_block (f32); every other unit: gelu_side (packed f16)

V_BO, V_G2, V_B2, V_B1, V_BFC2 = 0, 768, 1152, 1536, 3072  # vec_mlp offsets (kernels_block16.hip)
C1 = -2.0 * 0.79788456080286535588 * 1.44269504088896340736
C3 = C1 * 0.044715


def round16(x):
    """the allowance of one rounding of x to f16"""
    return np.maximum(U16 * np.abs(x), TINY16)


def f16(x):
    with np.errstate(over="ignore"):
        return np.asarray(x, np.float64).astype(np.float16).astype(np.float64)


def gelu_tanh(x):
    x = np.asarray(x, np.float64)
    return 0.5 * x * (1.0 + np.tanh(0.7978845608028654 * (x + 0.044715 * x ** 3)))


def gelu_f16_sequence(z):
    """`gelu_side` op by op on numpy float16 (z: float16 values, the converted pre-activations); exp2 and rcp correctly rounded"""
    h = np.float16
    with np.errstate(all="ignore"):
        c1, c3 = h(np.float32(C1)), h(np.float32(np.float32(C1) * np.float32(0.044715)))
        x = np.maximum(np.asarray(z, h), h(-65504.0))
        a = x * x
        a = (a.astype(np.float64) * np.float64(c3) + np.float64(c1)).astype(h)  # packed fma: one rounding
        a = a * x
        e = np.exp2(a.astype(np.float64)).astype(h)
        e = e + h(1.0)
        r = (1.0 / e.astype(np.float64)).astype(h)
        return x * r


_ENV = None


def gelu_envelope():
    """-> (largest |gelu_f16_sequence(z) - gelu(z)| / (u16 max(|z|, 1)) over every finite f16 z, the z it is reached at)"""
    global _ENV
    if _ENV is None:
        z = np.arange(65536, dtype=np.uint32).astype(np.uint16).view(np.float16)
        z = z[np.isfinite(z)]
        z64 = z.astype(np.float64)
        err = np.abs(gelu_f16_sequence(z).astype(np.float64) - gelu_tanh(z64)) / (U16 * np.maximum(np.abs(z64), 1.0))
        assert np.isfinite(err).all()
        i = int(np.argmax(err))
        _ENV = (float(err[i]), float(z64[i]))
    return _ENV


def gelu_allow(z, a_z):
    """allowance of a device hidden value (an f16) against the float64 gelu(z), apart from the 1.13 a_z the caller carries worst-case"""
    conv = round16(np.abs(z) + a_z)  # the f32 -> f16 conversion in front of the packed sequence
    return GELU_MARGIN * gelu_envelope()[0] * U16 * np.maximum(np.abs(z) + a_z + conv, 1.0) + GELU_LIPSCHITZ * conv


def gelu_grad(x):
    x = np.asarray(x, np.float64)
    with np.errstate(over="ignore"):
        s = 1.0 / (1.0 + np.exp(-2.0 * 0.7978845608028654 * (x + 0.044715 * x ** 3)))
    return s + x * s * (1.0 - s) * 2.0 * 0.7978845608028654 * (1.0 + 3 * 0.044715 * x * x)


def flips_through_mlp(dev, z, w1, w2, chunk=8):
    """sum_k |W2' diag(gelu'(z_m)) W1|[n, k] dev[m, k]: the LayerNorm flips of row m through the linearised MLP, worst case over their signs"""
    out = np.zeros((z.shape[0], w2.shape[0]))
    rows = np.flatnonzero(dev.any(axis=1))
    g = gelu_grad(z)
    for i in range(0, rows.size, chunk):
        r = rows[i:i + chunk]
        p = np.abs(np.matmul(w2[None] * g[r][:, None, :], w1))  # [rows, 384, 384]
        out[r] = np.einsum("cnk,ck->cn", p, dev[r])
    return out


def sum_allow(w, mag):
    """(K + 8) u32 mag per output column, K = nonzero weights of that output row"""
    return (np.count_nonzero(w, axis=1) + 8) * U32 * mag


def f16_deviation(v, e):
    """-> (f16(v), the largest distance of f16(v + d) from it over |d| <= e)"""
    r = f16(v)
    return r, np.maximum(f16(v + e) - r, r - f16(v - e))


def layer_norm(x, e_x, g, b, eps, width=D, rsq_rel=RSQ_REL, info=None):
    """-> (LN(x) float64, the allowance of the device's f32 value before any rounding to f16). `width`: the number of terms of the two row sums
    (the row kernels of tests/rows_ref.py pass their own C); `rsq_rel`: the relative error of the reciprocal root as the kernel forms it;
    `info`, a dict, receives t (per row) for callers that have to hold it inside the range the rstd bound is valid on."""
    mean = x.mean(axis=1, keepdims=True)
    d = x - mean
    var = (d * d).mean(axis=1, keepdims=True)
    a = g / np.sqrt(var + eps)
    e_mean = (width + 8) * U32 * np.abs(x).mean(axis=1, keepdims=True) + e_x.mean(axis=1, keepdims=True)
    e_d = e_x + e_mean
    e_var = (width + 8) * U32 * var + 2 * (np.abs(d) * e_d).mean(axis=1, keepdims=True) + (e_d * e_d).mean(axis=1, keepdims=True)
    t = e_var / (var + eps)
    if info is not None:
        info["t"] = t
    rel = rsq_rel + t / 2 + t * t
    allow = np.abs(a) * e_d + np.abs(d * a) * rel + 4 * U32 * (np.abs(x * a) + np.abs(mean * a) + np.abs(b))
    return d * a + b, allow


def flags(args):
    return args.get("att") is not None, bool(args.get("q")), bool(args.get("feat"))


def evaluate(args, guard_rows=ROW_GUARD, x_out=None):
    M, T, eps, qs = args["M"], args["T"], float(args["eps"]), float(args["q_scale"])
    mlp, qkv, tap = flags(args)
    f64 = lambda v: np.asarray(v).astype(np.float64)  # noqa: E731
    x_in = f64(args["x"]).reshape(M + guard_rows, D)
    x = x_in[:M]
    inter = {}

    def rows(val, allow, given):
        want, al, wr = np.zeros((M + guard_rows, D)), np.zeros((M + guard_rows, D)), np.zeros((M + guard_rows, D), bool)
        if given:
            want[:M], al[:M], wr[:M] = val, allow, True
        return want, al, wr

    e_x = np.zeros_like(x)
    out = {}
    if mlp and x_out is not None:  # the stages behind the MLP alone, on the stream the device wrote: nothing is carried into them
        x = f64(x_out).reshape(M + guard_rows, D)[:M]
    elif mlp:
        vm = f64(args["vec_mlp"])
        wo, w1, w2 = f64(args["wo"]), f64(args["w1"]), f64(args["w2"])
        att = f64(args["att"]).reshape(-1, D)[:M]
        bo, g2, b2, b1, bfc2 = vm[V_BO:V_BO + D], vm[V_G2:V_G2 + D], vm[V_B2:V_B2 + D], vm[V_B1:V_B1 + HID], vm[V_BFC2:V_BFC2 + D]
        x1 = x + bo + att @ wo.T
        a1 = sum_allow(wo, np.abs(att) @ np.abs(wo).T + np.abs(bo) + np.abs(x))
        ln, e_ln = layer_norm(x1, a1, g2, b2, eps)
        ln16, dev = f16_deviation(ln, e_ln)
        z = ln16 @ w1.T + b1
        s_z = sum_allow(w1, np.abs(ln16) @ np.abs(w1).T + np.abs(b1))
        a_z = s_z + dev @ np.abs(w1).T
        h = gelu_tanh(z)
        h16 = f16(h)
        a_g = gelu_allow(z, a_z) + np.abs(h16 - h) + GELU_LIPSCHITZ * s_z  # against the reference's own f16 hidden value
        x2 = x1 + bfc2 + h16 @ w2.T
        if args.get("fc2_random_signs", True):
            through = SIGMAS * np.sqrt((a_g * a_g) @ (w2 * w2).T)
        else:
            through = a_g @ np.abs(w2).T
        e_x = (a1 + sum_allow(w2, np.abs(h16) @ np.abs(w2).T + np.abs(bfc2) + np.abs(x1))
               + flips_through_mlp(dev, z, w1, w2) + (GELU_CURVATURE / 2 * a_z * a_z) @ np.abs(w2).T + through)
        out["cap_x1"] = rows(x1, a1, args.get("cap"))
        want_x, allow_x, written_x = rows(x2, e_x, True)
        want_x[M:] = x_in[M:]
        out["x"] = (want_x, allow_x, written_x)
        inter.update(x1=x1, a1=a1, ln2=ln, e_ln2=e_ln, dev_ln2=dev, z=z, a_z=a_z, h=h, a_h=gelu_allow(z, a_z) + GELU_LIPSCHITZ * a_z)
        x = x2
    else:
        out["cap_x1"] = rows(0, 0, False)
        out["x"] = (x_in.copy(), np.zeros_like(x_in), np.zeros(x_in.shape, bool))  # the QKV-only instance leaves the stream alone

    if tap:
        vt = f64(args["vec_tap"])
        ln, e_ln = layer_norm(x, e_x, vt[:D], vt[D:], eps)
        out["feat"] = rows(ln, e_ln + round16(np.abs(ln) + e_ln), True)
    else:
        out["feat"] = rows(0, 0, False)

    B = M // T if qkv else 1
    shape = (B + 1, HEADS, T if qkv else 1, 64)
    for name in "qkv":
        out[name] = (np.zeros(shape), np.zeros(shape), np.zeros(shape, bool))
    if qkv:
        vq, wq = f64(args["vec_qkv"]), f64(args["wqkv"])
        ln, e_ln = layer_norm(x, e_x, vq[:D], vq[D:2 * D], eps)
        ln16, dev = f16_deviation(ln, e_ln)
        bq = vq[2 * D:]
        y = ln16 @ wq.T + bq
        a_y = sum_allow(wq, np.abs(ln16) @ np.abs(wq).T + np.abs(bq)) + dev @ np.abs(wq).T
        inter.update(ln1=ln, e_ln1=e_ln, dev_ln1=dev)
        for i, name in enumerate("qkv"):
            sc = qs if i == 0 else 1.0
            v, e = y[:, i * D:(i + 1) * D] * sc, a_y[:, i * D:(i + 1) * D] * abs(sc)
            al = e + (U32 * np.abs(v) if i == 0 else 0.0) + round16(np.abs(v) + e)
            want, allow, written = out[name]
            want[:B] = v.reshape(B, T, HEADS, 64).transpose(0, 2, 1, 3)
            allow[:B] = al.reshape(B, T, HEADS, 64).transpose(0, 2, 1, 3)
            written[:B] = True
    out["_inter"] = inter
    return out

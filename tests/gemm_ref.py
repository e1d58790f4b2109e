"""float64 reference of vx_gemm_f16 and a derived per-element error allowance. Plain numpy, nothing from the device side.

`args` is a dict keyed by the fields of vx_gemm_args (include/visp_hip_kernels.h; `lambda_` for `lambda`), pointers replaced by numpy
arrays that hold the WHOLE buffer behind the pointer:
  A       f16 [rows, lda] (plain) or f16 [B, conv_H, conv_W, pix] (implicit conv; `A_off` = first channel of the slice A points at)
  W       f16 [N, K]          bias / lambda_ / noise  f32 vectors or None        pos  f32 [tokens_P + 1, N]
  res1    f16 [rows, ldo] (SILU: [rows, ld_res1])      res2  f16 [rows, ldo]      out0 f32 [M, ldo]: the RESID_F32 stream before the call
                                                                                  (guard rows after it start as zeros)
Every output buffer is described in full, as the call leaves a zero-initialised buffer: `evaluate` returns, per buffer name
("out", or "q" / "k" / "vt"), the expected content, the allowance of every element and which elements the call writes. The allowance of an
element the call must not write is 0, so one comparison `|got - want| <= bound` covers every element of every buffer.

The allowance (u16 = 2^-11, u32 = 2^-24; z = acc + bias, the value before the activation):
  accumulation   (K + 8) * u32 * (|A| @ |W|^T + |bias|): an f32 sum of K exact f16 x f16 products in ANY order is within (K - 1) u32 of the
                 exact sum times the sum of magnitudes, so it holds for whatever order the MFMA and a split-K use; the 8 spare units pay
                 for the bias add and the few f32 operations of an epilogue (noise add, 0.2 * t, * sqrt2, * q_scale, * lambda, + pos);
  f16 rounding   max(u16 * |x|, 2^-25) for each time a value x is rounded to f16 on the way out (2^-25: half the smallest subnormal);
  scaling        the accumulation term times the Lipschitz constant of what follows it (|lambda|, sqrt2, q_scale; 1 for ReLU);
  f32 outputs    no f16 rounding; the final f32 add rounds once more: 2 * u32 * (|x0| + |lambda * z|), likewise for TOKENS;
  GELU / SiLU / post_gelu   the device's exp / tanh approximations have no measured per-element bound: the project's F16_TOL = 4e-3 of the
                 largest reference magnitude, plus the bound above on the value before the activation (their Lipschitz constants are < 1.13).
HEAD_OUT's reference rounds conv2's output to f16 as the device does; the device's own copy can land on the neighbouring f16, so that
rounding is allowed twice, each weighted by |lambda[n]|, and the 32-term f32 dot product gets its own (N + 8) * u32 term."""
from __future__ import annotations

import numpy as np

U16, U32, TINY16 = 2.0 ** -11, 2.0 ** -24, 2.0 ** -25
F16_TOL = 4e-3  # tests/test_gpu_kernels.py

F16, GELU, RELU, RESID_F32, TOKENS, QKV, PIXSHUF, ADD, HEAD_OUT, LRELU_AGC, SILU = range(11)
EPI_NAMES = ["F16", "F16_GELU", "F16_RELU", "RESID_F32", "TOKENS", "QKV", "PIXSHUF", "F16_ADD", "HEAD_OUT", "LRELU_AGC", "SILU"]
F32_OUT = (RESID_F32, TOKENS, HEAD_OUT)
SQRT2 = 2.0 ** 0.5


def _get(args, key, default=0):
    v = args.get(key)
    return default if v is None else v


def f64(a):
    return np.asarray(a, np.float64)


def gelu_tanh(x):
    return 0.5 * x * (1.0 + np.tanh(0.7978845608028654 * (x + 0.044715 * x ** 3)))


def silu(x):
    return x / (1.0 + np.exp(-x))


def round16(x):
    """the allowance of one rounding of x to f16"""
    return np.maximum(U16 * np.abs(x), TINY16)


def a_matrix(args) -> np.ndarray:
    """The [M, K] matrix the A loader presents: plain rows (lda, row remap) or the im2col of an NHWC map; k past kh*kw*Cin is zero."""
    M, K = args["M"], args["K"]
    A = args["A"]
    m = np.arange(M)
    if _get(args, "conv_kh") > 0:
        kh, kw, s, p = args["conv_kh"], args["conv_kw"], args["conv_stride"], args["conv_pad"]
        H, Wd, cin, OH, OW = args["conv_H"], args["conv_W"], args["conv_Cin"], args["conv_OH"], args["conv_OW"]
        c0 = _get(args, "A_off")
        pix = _get(args, "conv_pix") or cin
        assert A.shape[1:] == (H, Wd, pix) and c0 + cin <= pix
        x = f64(A[..., c0:c0 + cin])
        b, rm = m // (OH * OW), m % (OH * OW)
        oy, ox = rm // OW, rm % OW
        out = np.zeros((M, K))
        for tap in range(kh * kw):
            ky, kx = divmod(tap, kw)
            iy, ix = oy * s - p + ky, ox * s - p + kx
            ok = (iy >= 0) & (iy < H) & (ix >= 0) & (ix < Wd)
            out[ok, tap * cin:(tap + 1) * cin] = x[b[ok], iy[ok], ix[ok]]
    else:
        g = _get(args, "a_group")
        rows = m if g <= 0 else (m // g) * args["a_group_stride"] + args["a_row_off"] + m % g
        assert A.ndim == 2 and A.shape[1] == args["lda"]
        out = f64(A[rows, :K])
    if _get(args, "a_relu"):
        out = np.maximum(out, 0.0)
    return out


def window_pixel_rows(M, ws, res_w, res_h, shift):
    """Row m of a window-ordered product (window_partition of the zero-padded, rolled map) -> pixel row of the [B, res_h, res_w] map, or -1
    for a row of the padding: window_reverse, roll(+shift) over the padded extent, crop."""
    res_h = res_h if res_h > 0 else res_w
    nwx, nwy = -(-res_w // ws), -(-res_h // ws)
    m = np.arange(M)
    inner, win = m % (ws * ws), m // (ws * ws)
    wx, wy, b = win % nwx, (win // nwx) % nwy, win // (nwx * nwy)
    py = (wy * ws + inner // ws + shift) % (nwy * ws)
    px = (wx * ws + inner % ws + shift) % (nwx * ws)
    return np.where((py < res_h) & (px < res_w), (b * res_h + py) * res_w + px, -1)


def out_rows(args) -> int:
    """rows of the row-major `out` buffer (and of res1 / res2)"""
    if _get(args, "win_ws") > 0:
        rh = _get(args, "win_res_h") or args["win_res"]
        nw = -(-args["win_res"] // args["win_ws"]) * -(-rh // args["win_ws"])
        return args["M"] // (nw * args["win_ws"] ** 2) * rh * args["win_res"]
    return args["M"]


def evaluate(args, guard_rows=0):
    """-> (want, allow, written): three dicts, buffer name -> array of the buffer's full shape (float64, float64, bool).
    `guard_rows` appends that many rows to every row-major `out` buffer, past the last row the call owns: they start as zeros, no element of
    them is written and their allowance is 0, so a store from a tile's rows >= M shows up in the comparison instead of past the allocation."""
    M, N, K, epi = args["M"], args["N"], args["K"], args["epi"]
    Am, W = a_matrix(args), f64(args["W"])
    assert W.shape == (N, K)
    bias = f64(args["bias"]) if args.get("bias") is not None else np.zeros(N)
    z = Am @ W.T + bias
    mag = np.abs(Am) @ np.abs(W).T + np.abs(bias)
    nv = _get(args, "n_valid") or N
    ldo = _get(args, "ldo")
    m = np.arange(M)

    if epi == LRELU_AGC and args.get("noise") is not None:
        nz = f64(args["noise"])[m % args["noise_hw"]][:, None]
        z, mag = z + nz, mag + np.abs(nz)
    acc = (K + 8) * U32 * mag

    def rows_buffer(val, allow, rows=None, n_rows=None, dtype_f16=True):
        n_rows = n_rows if n_rows is not None else M + guard_rows
        rows = m if rows is None else rows
        keep = rows >= 0
        want, al, wr = np.zeros((n_rows, ldo)), np.zeros((n_rows, ldo)), np.zeros((n_rows, ldo), bool)
        want[rows[keep], :nv], al[rows[keep], :nv], wr[rows[keep], :nv] = val[keep, :nv], allow[keep, :nv], True
        return {"out": want}, {"out": al}, {"out": wr}

    def res(name, rows=None, ld=None):
        r = args.get(name)
        if r is None:
            return None
        rows = m if rows is None else np.maximum(rows, 0)
        assert r.shape[1] == (ld or ldo)
        out = np.zeros((M, N))
        out[:, :nv] = f64(r[rows, :nv])
        return out

    if epi in (F16, RELU):
        val = np.maximum(z, 0.0) if epi == RELU else z
        return rows_buffer(val, acc + round16(val))
    if epi == GELU:
        val = gelu_tanh(z)
        return rows_buffer(val, F16_TOL * np.abs(val[:, :nv]).max() + acc + round16(z))
    if epi == SILU:
        act = silu(z)
        r1 = res("res1", ld=_get(args, "ld_res1") or ldo)
        val = act if r1 is None else act + r1
        allow = F16_TOL * np.abs(val[:, :nv]).max() + acc + round16(z)
        return rows_buffer(val, allow if r1 is None else allow + round16(val))
    if epi == LRELU_AGC:
        act = np.clip(np.where(z < 0, 0.2 * z, z) * SQRT2, -256.0, 256.0)
        r1 = res("res1")
        val = act if r1 is None else act + r1
        allow = SQRT2 * acc + round16(act)
        return rows_buffer(val, allow if r1 is None else allow + round16(val))
    if epi == ADD:
        rows, n_rows = None, None
        if _get(args, "win_ws") > 0:
            rows = window_pixel_rows(M, args["win_ws"], args["win_res"], _get(args, "win_res_h"), _get(args, "win_shift"))
            n_rows = out_rows(args) + guard_rows
        t = np.maximum(z, 0.0) if _get(args, "relu") else z
        r1, r2 = res("res1", rows), res("res2", rows)
        pre = t + (0 if r1 is None else r1) + (0 if r2 is None else r2)
        allow = acc + round16(t)
        if _get(args, "post_gelu"):
            val = gelu_tanh(pre)
            allow = F16_TOL * np.abs(val[:, :nv]).max() + allow + round16(pre)
        else:
            val = pre
            if r1 is not None:
                allow = allow + round16(val)
        return rows_buffer(val, allow, rows, n_rows)
    if epi == RESID_F32:
        lam, x0 = f64(args["lambda_"]), f64(args["out0"])
        assert nv == N and x0.shape == (M, ldo)
        want, al, wr = np.zeros((M + guard_rows, ldo)), np.zeros((M + guard_rows, ldo)), np.zeros((M + guard_rows, ldo), bool)
        want[:M] = x0
        want[:M, :N] += lam * z
        al[:M, :N] = np.abs(lam) * acc + 2 * U32 * (np.abs(x0[:, :N]) + np.abs(lam * z))
        wr[:M, :N] = True
        return {"out": want}, {"out": al}, {"out": wr}
    if epi == TOKENS:
        P, pos = args["tokens_P"], f64(args["pos"])
        assert nv == N
        n_img = -(-(M + guard_rows) // P)  # the scattered layouts hold whole images: enough of them that rows M .. M + guard_rows have a place
        rows = (m // P) * (P + 1) + 1 + m % P
        pz = pos[1 + m % P]
        return rows_buffer(z + pz, acc + 2 * U32 * (np.abs(z) + np.abs(pz)), rows, n_img * (P + 1))
    if epi == QKV:
        T, Hh = args["qkv_T"], args["qkv_H"]
        C = Hh * 64
        assert N == 3 * C
        n_img = -(-(M + guard_rows) // T)
        b, t = m // T, m % T
        want, al, wr = {}, {}, {}
        for i, name in enumerate(("q", "k", "vt")):
            sc = float(args["q_scale"]) if i == 0 else 1.0
            val = (z[:, i * C:(i + 1) * C] * sc).reshape(M, Hh, 64)
            allow = abs(sc) * acc[:, i * C:(i + 1) * C].reshape(M, Hh, 64) + round16(val)
            want[name], al[name], wr[name] = np.zeros((n_img, Hh, T, 64)), np.zeros((n_img, Hh, T, 64)), np.zeros((n_img, Hh, T, 64), bool)
            want[name][b, :, t], al[name][b, :, t], wr[name][b, :, t] = val, allow, True
        return want, al, wr
    if epi == PIXSHUF:
        s, co, Hh, Ww = args["ps_s"], args["ps_Cout"], args["ps_H"], args["ps_W"]
        assert nv == s * s * co
        n_img = -(-(M + guard_rows) // (Hh * Ww))
        b, rm = m // (Hh * Ww), m % (Hh * Ww)
        y, x = rm // Ww, rm % Ww
        shape = (n_img, Hh * s, Ww * s, ldo)
        want, al, wr = np.zeros(shape), np.zeros(shape), np.zeros(shape, bool)
        allow = acc + round16(z)
        for tap in range(s * s):
            dy, dx = divmod(tap, s)
            cols = slice(tap * co, (tap + 1) * co)
            want[b, y * s + dy, x * s + dx, :co], al[b, y * s + dy, x * s + dx, :co] = z[:, cols], allow[:, cols]
            wr[b, y * s + dy, x * s + dx, :co] = True
        return {"out": want}, {"out": al}, {"out": wr}
    if epi == HEAD_OUT:
        lam, hb, hs = f64(args["lambda_"]), float(args["head_bias"]), float(args["head_scale"])
        assert N == 32
        t = np.maximum(z, 0.0)
        h2 = f64(t.astype(np.float16))  # conv2's output as the fused kernel holds it
        y = h2 @ lam + hb
        allow = abs(hs) * ((acc + 2 * round16(t)) @ np.abs(lam) + (N + 8) * U32 * (np.abs(h2) @ np.abs(lam) + abs(hb)))
        pad = np.zeros(guard_rows)  # one f32 per row
        return {"out": np.append(np.maximum(y, 0.0) * hs, pad)}, {"out": np.append(allow, pad)}, {"out": np.append(np.ones(M, bool), pad > 0)}
    raise ValueError(f"unknown epilogue {epi}")


def gemm_ref(args):
    return evaluate(args)[0]


def bound(args):
    return evaluate(args)[1]

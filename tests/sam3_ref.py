"""float64 numpy reference of the SAM3 vision encoder and the CLIP text encoder as the reference's graph builds them (src/visp/arch/sam3.h), and numpy
emulations of the two new copy kernels. Written from the formulas of the ROPE op (include/visp_c_api.h) and the reference's node order; pinned to
`transformers` by tests/test_sam3_ref_cpu.py.

Arrays are in numpy order (the reverse of ggml's ne): activations [B, T, C] or [B, H, W, C], q / k / v [B, T, heads, head_dim]. `w` maps the converter's tensor
names to arrays as the weight store presents them (synth.sam3_graph_tensors): linear [out, in], conv [Cout, kh, kw, Cin], conv_transpose [Cin, Cout, kh, kw].
Every function takes `rnd`, applied to each node's output: the identity for the exact reference, `f16` for the pipeline's f16 floor -- a rounding wherever the
per-node plan of the executor holds an f16 buffer."""
from __future__ import annotations

import math

import numpy as np


def f16(x):
    return np.asarray(x, np.float64).astype(np.float16).astype(np.float64)


def exact(x):
    return np.asarray(x, np.float64)


# ---- ROPE ----------------------------------------------------------------------------------------------------------------------------------------------------

def rope_angles(pos, n_dims: int, base: float, scale: float) -> np.ndarray:
    """theta[t, i] = pos[t] * scale * base^(-2 i / n) for pair i in [0, n / 2)."""
    i = np.arange(n_dims // 2, dtype=np.float64)
    return np.asarray(pos, np.float64)[:, None] * (float(scale) * np.power(float(base), -2.0 * i / n_dims))[None, :]


def rope(x, pos, n_dims: int, base: float, scale: float) -> np.ndarray:
    """ggml_rope_ext, GGML_ROPE_TYPE_NORMAL: x [B, T, heads, n], pos [T]; out[2i] = x[2i] cos - x[2i+1] sin, out[2i+1] = x[2i] sin + x[2i+1] cos."""
    x = np.asarray(x, np.float64)
    assert x.shape[-1] == n_dims and x.shape[1] == len(pos)
    th = rope_angles(pos, n_dims, base, scale)
    c, s = np.cos(th)[None, :, None, :], np.sin(th)[None, :, None, :]
    out = np.empty_like(x)
    out[..., 0::2] = x[..., 0::2] * c - x[..., 1::2] * s
    out[..., 1::2] = x[..., 0::2] * s + x[..., 1::2] * c
    return out


def rope_2d(x, px, py, base: float, scale: float, rnd=exact) -> np.ndarray:
    """apply_rope_2d (sam3.h:413-438): x positions on the first half of a head, y positions on the second."""
    h = x.shape[-1] // 2
    first = rnd(rope(rnd(x[..., :h]), px, h, base, scale))
    second = rnd(rope(rnd(x[..., h:]), py, h, base, scale))
    return rnd(np.concatenate([first, second], -1))


def rope_table(pos, n: int, base: float, scale: float) -> np.ndarray:
    """The lowering's table: f32 [T][n], cos | sin of the angles computed in double."""
    th = rope_angles(pos, n, base, scale)
    return np.concatenate([np.cos(th), np.sin(th)], 1).astype(np.float32)


def emulate_rope_kernel(x16: np.ndarray, table: np.ndarray, q_scale: float = 1.0, variant: str = "") -> np.ndarray:
    """vx_rope_f16 step by step: f16 in, f32 table, f32 arithmetic (a product, an fma, the scale), one f16 rounding. x16 [B, T, heads, n] f16. `variant` models a
    wrong kernel (for the tests that show the allowance tells them apart)."""
    f32 = np.float32
    n = x16.shape[-1]
    x = x16.astype(f32)
    co, sn = table[:, : n // 2][None, :, None, :], table[:, n // 2:][None, :, None, :]
    x0, x1 = x[..., 0::2], x[..., 1::2]
    if variant == "rotate_half":  # pairs (i, i + n / 2) instead of (2i, 2i + 1)
        x0, x1 = x[..., : n // 2], x[..., n // 2:]
    if variant == "sin_sign":
        sn = -sn
    # fmaf(-x1, sn, x0 * co): the product is rounded to f32, the fma once more
    a = ((x0 * co).astype(f32).astype(np.float64) - x1.astype(np.float64) * sn.astype(np.float64)).astype(f32)
    b = ((x0 * sn).astype(f32).astype(np.float64) + x1.astype(np.float64) * co.astype(np.float64)).astype(f32)
    a, b = (a * f32(q_scale)).astype(f32), (b * f32(q_scale)).astype(f32)
    out = np.empty(x.shape, np.float16)
    if variant == "rotate_half":
        out[..., : n // 2], out[..., n // 2:] = a.astype(np.float16), b.astype(np.float16)
    else:
        out[..., 0::2], out[..., 1::2] = a.astype(np.float16), b.astype(np.float16)
    return out


def rope_allowance(ref: np.ndarray, x16: np.ndarray, q_scale: float) -> np.ndarray:
    """Per element: 2^-11 |ref| (one f16 rounding) + 2^-21 (|x0| + |x1|) |q_scale| (at most five f32 roundings of terms no larger than that, covered by
    eight) + 2^-25 (the f16 subnormal step)."""
    x = np.abs(x16.astype(np.float64))
    mag = np.empty_like(x)
    mag[..., 0::2] = mag[..., 1::2] = x[..., 0::2] + x[..., 1::2]
    return 2.0 ** -11 * np.abs(ref) + 2.0 ** -21 * mag * abs(q_scale) + 2.0 ** -25


def emulate_get_rows_kernel(table16: np.ndarray, idx: np.ndarray) -> np.ndarray:
    """vx_get_rows_f16: out[j] = table[idx[j]], a row of zeros for an index outside [0, rows) (which never reads)."""
    rows = table16.shape[0]
    idx = np.asarray(idx)
    ok = (idx >= 0) & (idx < rows)
    out = np.zeros(idx.shape + (table16.shape[1],), table16.dtype)
    out[ok] = table16[idx[ok]]
    return out


# ---- nn ------------------------------------------------------------------------------------------------------------------------------------------------------

def linear(w, name, x, rnd=exact):
    y = x @ np.asarray(w[name + ".weight"], np.float64).T
    if name + ".bias" in w:
        y = y + np.asarray(w[name + ".bias"], np.float64)
    return rnd(y)


def layer_norm(w, name, x, rnd=exact, eps=1e-5):
    mu = x.mean(-1, keepdims=True)
    var = ((x - mu) ** 2).mean(-1, keepdims=True)
    return rnd((x - mu) / np.sqrt(var + eps) * np.asarray(w[name + ".weight"], np.float64) + np.asarray(w[name + ".bias"], np.float64))


def gelu(x, rnd=exact):  # ggml_gelu: the tanh form
    return rnd(0.5 * x * (1.0 + np.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * x ** 3))))


def attention(q, k, v, mask, scale):
    """q, k, v [B, T, heads, hd]; mask None or [T_q, T_k] of 0 / -inf -> [B, T, heads * hd]."""
    s = np.einsum("bqhd,bkhd->bhqk", q, k) * scale
    if mask is not None:
        s = s + np.asarray(mask, np.float64)[None, None]
    s = s - s.max(-1, keepdims=True)
    p = np.exp(s)
    p = p / p.sum(-1, keepdims=True)
    o = np.einsum("bhqk,bkhd->bqhd", p, v)
    return o.reshape(o.shape[0], o.shape[1], -1)


def conv_2d(w, name, x, stride=1, pad=0, rnd=exact):
    """x [B, H, W, Cin], weight [Cout, kh, kw, Cin]."""
    k = np.asarray(w[name + ".weight"], np.float64)
    co, kh, kw, ci = k.shape
    if pad:
        x = np.pad(x, ((0, 0), (pad, pad), (pad, pad), (0, 0)))
    B, H, W, _ = x.shape
    oh, ow = (H - kh) // stride + 1, (W - kw) // stride + 1
    y = np.zeros((B, oh, ow, co))
    for dy in range(kh):
        for dx in range(kw):
            y += x[:, dy:dy + stride * oh:stride, dx:dx + stride * ow:stride, :] @ k[:, dy, dx, :].T
    if name + ".bias" in w:
        y = y + np.asarray(w[name + ".bias"], np.float64)
    return rnd(y)


def conv_transpose_2d(w, name, x, stride, rnd=exact):
    """kernel == stride; x [B, H, W, Cin], weight [Cin, Cout, k, k] -> [B, k H, k W, Cout]."""
    k = np.asarray(w[name + ".weight"], np.float64)
    ci, co, kh, kw = k.shape
    assert kh == stride and kw == stride
    B, H, W, _ = x.shape
    y = np.einsum("bhwi,ioyx->bhywxo", x, k).reshape(B, H * kh, W * kw, co)
    if name + ".bias" in w:
        y = y + np.asarray(w[name + ".bias"], np.float64)
    return rnd(y)


def max_pool_2x2(x):
    B, H, W, C = x.shape
    return x[:, : H // 2 * 2, : W // 2 * 2].reshape(B, H // 2, 2, W // 2, 2, C).max((2, 4))


# ---- vision side (sam3.h:313-613) ------------------------------------------------------------------------------------------------------------------------

def rope_2d_positions(n_pos: int, n_rows: int):
    i = np.arange(n_pos)
    return i % n_rows, i // n_rows


def window_partition(x, window):
    B, H, W, C = x.shape
    py, px = (window - H % window) % window, (window - W % window) % window
    x = np.pad(x, ((0, 0), (0, py), (0, px), (0, 0)))
    nh, nw = (H + py) // window, (W + px) // window
    x = x.reshape(B, nh, window, nw, window, C).transpose(0, 1, 3, 2, 4, 5)
    return x.reshape(B * nh * nw, window * window, C)


def window_reverse(x, H, W, window, B):
    py, px = (window - H % window) % window, (window - W % window) % window
    nh, nw = (H + py) // window, (W + px) // window
    x = x.reshape(B, nh, nw, window, window, -1).transpose(0, 1, 3, 2, 4, 5).reshape(B, H + py, W + px, -1)
    return x[:, :H, :W]


def rope_attention(w, p, x, heads, pos, rnd=exact):
    """x [B, T, C]; pos = (px, py, scale)."""
    B, T, C = x.shape
    hd = C // heads
    q, k, v = (linear(w, f"{p}.{n}", x, rnd).reshape(B, T, heads, hd) for n in ("q_proj", "k_proj", "v_proj"))
    q, k = rope_2d(q, pos[0], pos[1], 10000.0, pos[2], rnd), rope_2d(k, pos[0], pos[1], 10000.0, pos[2], rnd)
    return linear(w, f"{p}.o_proj", rnd(attention(q, k, v, None, 1.0 / math.sqrt(hd))), rnd)


def vision_layer(w, p, x, window, heads, pos, rnd=exact):
    """x [B, H, W, C] (sam3.h:457-483)."""
    B, H, W, C = x.shape
    res = x
    x = layer_norm(w, f"{p}.layer_norm1", x, rnd)
    x = rnd(window_partition(x, window)) if window > 0 else x.reshape(B, H * W, C)
    x = rope_attention(w, f"{p}.attention", x, heads, pos, rnd)
    x = rnd(window_reverse(x, H, W, window, B)) if window > 0 else x.reshape(B, H, W, C)
    x = rnd(x + res)
    y = layer_norm(w, f"{p}.layer_norm2", x, rnd)
    y = linear(w, f"{p}.mlp.fc2", gelu(linear(w, f"{p}.mlp.fc1", y, rnd), rnd), rnd)
    return rnd(y + x)


def vision_embed(w, p, image, patch, rnd=exact):
    """image [B, H, W, 3] f32 -> [B, H / patch, W / patch, C] (sam3.h:313-338)."""
    x = conv_2d(w, f"{p}.patch_embeddings.projection", np.asarray(image, np.float64), patch, 0, rnd)
    B, hp, wp, C = x.shape
    pos = np.asarray(w[f"{p}.position_embeddings"], np.float64).reshape(-1, C)
    n = int(math.sqrt(pos.shape[0]) + 0.5)
    pos = pos.reshape(n, n, C)
    if (hp, wp) != (n, n):  # ggml_repeat: out[i] = src[i mod n]
        pos = pos[np.arange(hp)[:, None] % n, np.arange(wp)[None, :] % n]
    return rnd(x + pos[None])


def vision_transformer(w, p, image, params, rnd=exact):
    """params: synth.Sam3VitConfig-like (patch, window, image_size, n_layers, heads, global_layers). -> [B, H, W, C]"""
    x = vision_embed(w, f"{p}.embeddings", image, params.patch, rnd)
    wx, wy = rope_2d_positions(params.window ** 2, params.window)
    n_glob = params.image_size // params.patch
    gx, gy = rope_2d_positions(n_glob ** 2, n_glob)
    x = layer_norm(w, f"{p}.layer_norm", x, rnd)
    for i in range(params.n_layers):
        glob = i in params.global_layers
        pos = (gx, gy, float(params.window) / float(n_glob)) if glob else (wx, wy, 1.0)
        x = vision_layer(w, f"{p}.layers.{i}", x, 0 if glob else params.window, params.heads, pos, rnd)
    return x


def sine_position_embedding(width, height, n_pos_feats, normalize=True):
    """sam3.h:524-564 in float64: [H, W, 2 F] (CWHN order), y features first."""
    k = np.arange(n_pos_feats)
    dim_t = 10000.0 ** (2.0 * (k // 2) / n_pos_feats)
    y, x = np.arange(1, height + 1, dtype=np.float64), np.arange(1, width + 1, dtype=np.float64)
    if normalize:
        y, x = y / (height + 1e-6) * 2.0 * math.pi, x / (width + 1e-6) * 2.0 * math.pi
    ay, ax = y[:, None] / dim_t, x[:, None] / dim_t
    fy, fx = np.where(k % 2 == 0, np.sin(ay), np.cos(ay)), np.where(k % 2 == 0, np.sin(ax), np.cos(ax))
    out = np.empty((height, width, 2 * n_pos_feats))
    out[..., :n_pos_feats], out[..., n_pos_feats:] = fy[:, None, :], fx[None, :, :]
    return out


def fpn_layer(w, p, x, index, rnd=exact):
    if index == 0:
        x = conv_transpose_2d(w, f"{p}.scale_layers.0", x, 2, rnd)
        x = gelu(x, rnd)
        x = conv_transpose_2d(w, f"{p}.scale_layers.2", x, 2, rnd)
    elif index == 1:
        x = conv_transpose_2d(w, f"{p}.scale_layers.0", x, 2, rnd)
    elif index == 3:
        x = max_pool_2x2(x)
    x = conv_2d(w, f"{p}.proj1", x, 1, 0, rnd)
    return conv_2d(w, f"{p}.proj2", x, 1, 1, rnd)


def vision_neck(w, p, x, rnd=exact):
    hidden = [fpn_layer(w, f"{p}.fpn_layers.{i}", x, i, rnd) for i in range(4)]
    pos = [sine_position_embedding(h.shape[2], h.shape[1], h.shape[3] // 2, True) for h in hidden]
    return hidden, pos


def encode_vision(w, p, image, params, rnd=exact):
    return vision_neck(w, f"{p}.neck", vision_transformer(w, f"{p}.backbone", image, params, rnd), rnd)


# ---- text side (sam3.h:221-288) ------------------------------------------------------------------------------------------------------------------------------

def clip_encode_text(w, p, ids, mask, heads, rnd=exact):
    """ids [B, T] int, mask [T, T] of 0 / -inf -> [B, T, C] (final_layer_norm applied)."""
    ids = np.asarray(ids)
    B, T = ids.shape
    x = rnd(np.asarray(w[f"{p}.embeddings.token_embedding.weight"], np.float64))[ids]  # (the gather's f16 table image)
    x = rnd(x + np.asarray(w[f"{p}.embeddings.position_embedding.weight"], np.float64)[:T][None])
    i = 0
    while f"{p}.encoder.layers.{i}.layer_norm1.weight" in w:
        lp = f"{p}.encoder.layers.{i}"
        C = x.shape[-1]
        hd = C // heads
        y = layer_norm(w, f"{lp}.layer_norm1", x, rnd)
        q, k, v = (linear(w, f"{lp}.self_attn.{n}", y, rnd).reshape(B, T, heads, hd) for n in ("q_proj", "k_proj", "v_proj"))
        y = linear(w, f"{lp}.self_attn.out_proj", rnd(attention(q, k, v, mask, 1.0 / math.sqrt(hd))), rnd)
        x = rnd(y + x)
        y = layer_norm(w, f"{lp}.layer_norm2", x, rnd)
        y = linear(w, f"{lp}.mlp.fc2", gelu(linear(w, f"{lp}.mlp.fc1", y, rnd), rnd), rnd)
        x = rnd(y + x)
        i += 1
    return layer_norm(w, f"{p}.final_layer_norm", x, rnd)


def encode_text(w, p, ids, mask, heads, rnd=exact):
    return linear(w, f"{p}.text_projection", clip_encode_text(w, f"{p}.te.text_model", ids, mask, heads, rnd), rnd)


# ---- the kernel cases of tests/test_gpu_graph_sam3.py, checked against the emulation on the CPU by tests/test_sam3_ref_cpu.py ----------------------------------

VX_ATTN_Q_SCALE = 0.18033688011112042  # log2(e) / sqrt(64), include/visp_hip_kernels.h


def _grid(w, h):
    return rope_2d_positions(w * h, w)


def _arbitrary(n, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 72, n), rng.integers(0, 72, n)


# (name, head_dim, heads, T, B, (px, py), freq_scale): whole heads through vx_rope2d_f16; every half of them also through vx_rope_f16 (n = 32)
ROPE_CASES = [
    ("one", 64, 1, 1, 1, _grid(1, 1), 1.0),
    ("window4x4", 64, 2, 16, 3, _grid(4, 4), 1.0),
    ("odd5x5", 64, 3, 25, 2, _grid(5, 5), 1.0),
    ("global8x8", 64, 2, 64, 1, _grid(8, 8), 0.5),
    ("sam3_window", 64, 16, 576, 2, _grid(24, 24), 1.0),
    ("arbitrary", 64, 2, 40, 1, _arbitrary(40, 5), 1.0 / 3.0),
]
ROPE_BASE = 10000.0


def rope_case_data(case, seed=0):
    """Standard normal f16 q and k [B, T, heads, hd] of a case."""
    _, hd, heads, T, B, _, _ = case
    rng = np.random.default_rng(1000 + seed + T)
    return rng.standard_normal((B, T, heads, hd)).astype(np.float16), rng.standard_normal((B, T, heads, hd)).astype(np.float16)

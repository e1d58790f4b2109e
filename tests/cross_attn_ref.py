"""float64 numpy references for the graph layer's attention_cross, mul_mat, sin / cos and Fourier-feature kernels (kernels_attn_cross.hip,
kernels_samdec.hip), on f16-rounded operands, in the layouts the kernels take: token-major attention rows, ggml's mul_mat, f32 coordinates."""
import numpy as np


def f16(a):
    """the f16 rounding of a, as float64"""
    return np.asarray(a, np.float64).astype(np.float16).astype(np.float64)


def rel_err(got, want):
    """largest absolute error over the largest reference value"""
    return float(np.abs(np.asarray(got, np.float64) - want).max() / np.abs(want).max())


def f16_floor(want):
    """what rounding the exact result to f16 costs on its own: the floor of any comparison with an f16 output"""
    return rel_err(f16(want), want)


# the attention cases of the issue: (head_dim, heads, T_q, T_k, B, factor on q). The key split cuts T_k >= 256 into parts of 128 when T_q <= 32: 333 keys are
# two full parts and a tail of 77 (no multiple of 32); 255 / 256 are the two sides of the threshold; (16, 1, 33, 300, 1): many keys, but too many queries to split
ATTENTION_CASES = [(16, 1, 1, 1, 1, 1.0), (32, 3, 7, 7, 2, 1.0), (16, 2, 7, 333, 2, 1.0), (16, 8, 7, 4096, 1, 1.0), (16, 2, 333, 7, 2, 1.0), (32, 2, 50, 77, 1, 1.0),
                   (64, 1, 33, 65, 2, 1.0), (16, 2, 7, 333, 1, 6.0)]
SPLIT_EDGE_CASES = [(32, 1, 32, 255, 1, 1.0), (32, 1, 32, 256, 1, 1.0), (64, 2, 5, 300, 1, 1.0), (16, 1, 33, 300, 1, 1.0)]
MUL_MAT_CASES = [(8, 1, 1, 1, 1), (32, 100, 4, 2, 2), (64, 257, 5, 1, 1), (32, 4096, 4, 1, 1), (256, 300, 16, 2, 1)]  # (K, M, N, B, Ba); the last: Ba = 1 on B = 2, both limits


def attention_operands(case, seed=0):
    """standard normal q [B, T_q, H, hd] (times the case's factor), k, v [B, T_k, H, hd], as f16"""
    hd, H, Tq, Tk, B, qf = case
    rng = np.random.default_rng(seed)
    q = (rng.standard_normal((B, Tq, H, hd)) * qf).astype(np.float16)
    k = rng.standard_normal((B, Tk, H, hd)).astype(np.float16)
    v = rng.standard_normal((B, Tk, H, hd)).astype(np.float16)
    return q, k, v


def attention(q, k, v, scale):
    """q [B, T_q, H, hd], k, v [B, T_k, H, hd] -> [B, T_q, H * hd] = softmax(scale q k^T) v per head"""
    q, k, v = (np.asarray(t, np.float64) for t in (q, k, v))
    B, Tq, H, hd = q.shape
    s = np.einsum("bqhd,bkhd->bhqk", q, k) * scale
    s -= s.max(-1, keepdims=True)
    p = np.exp(s)
    p /= p.sum(-1, keepdims=True)
    return np.einsum("bhqk,bkhd->bqhd", p, v).reshape(B, Tq, H * hd)


def attention_bound(want):
    """the masked attention's rule: max(4 x the f16 floor, 4e-3) of the largest output"""
    return max(4 * f16_floor(want), 4e-3)


def mul_mat(a, b):
    """ggml_mul_mat: a [Ba, M, K], b [B, N, K] -> [B, N, M] (ne [M, N, B]); Ba is 1 or B"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.einsum("bmk,bnk->bnm", np.broadcast_to(a, (b.shape[0],) + a.shape[1:]), b)


def fourier_features(coords, gauss):
    """coords f32 [..., 2], gauss [2, F] (f16-rounded by the caller) -> [..., 2 F] = sin | cos of 2 pi (x g0 + y g1)"""
    t = 2.0 * np.pi * (np.asarray(coords, np.float64) @ np.asarray(gauss, np.float64))
    return np.concatenate([np.sin(t), np.cos(t)], -1)

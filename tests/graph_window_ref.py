"""float64 numpy references of the graph layer's window ops (PERMUTE / ROLL / PAD / ATTENTION_MASKED, split_qkv) on f16-rounded
operands, with ggml's conventions: a tensor of ne [n0, n1, n2, n3] is the numpy array of shape (n3, n2, n1, n0)."""
import numpy as np


def f16(a):
    """The values an f16 tensor holds, as float64."""
    return np.asarray(a, np.float32).astype(np.float16).astype(np.float64)


def rel_err(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float(np.abs(got - want).max() / np.abs(want).max())


def permute(x, axes):
    """ggml_permute(x, a0..a3) made contiguous: source dimension d becomes dimension axes[d]. x: numpy, shape = reversed ne (4-D)."""
    assert x.ndim == 4
    # numpy axis of ggml dimension d is 3 - d; result ggml dimension axes[d] takes source dimension d
    order = [0] * 4
    for d, a in enumerate(axes):
        order[3 - a] = 3 - d
    return np.ascontiguousarray(x.transpose(order))


def roll(x, shifts):
    """ggml_roll: dst[i] = src[(i - s) mod n] per dimension = numpy.roll with the same shifts."""
    return np.roll(x, tuple(shifts), tuple(3 - d for d in range(4)))


def pad(x, pads):
    """ggml_pad: zeros appended at the end of each dimension."""
    return np.pad(x, [(0, pads[3 - ax]) for ax in range(4)])


def attention_masked(q, k, v, mask, scale):
    """q, k, v: [B, T, H, hd] (ne [hd, H, T, B]); mask: [Bm, Hm, T_q, T_k] (ne [T_k, T_q, Hm, Bm]), -inf allowed; batch b reads mask b % Bm,
    Hm = 1 broadcasts over the heads. float64 throughout. Returns [B, T, H * hd] (ne [hd * H, T, B])."""
    q, k, v, mask = (np.asarray(a, np.float64) for a in (q, k, v, mask))
    B, T, H, hd = q.shape
    Bm, Hm = mask.shape[:2]
    assert B % Bm == 0 and Hm in (1, H)
    s = np.einsum("bihd,bjhd->bhij", q, k) * scale + mask[np.arange(B) % Bm]  # [B, Hm -> H, T, T]
    s = s - s.max(-1, keepdims=True)
    p = np.exp(s)
    p /= p.sum(-1, keepdims=True)
    return np.einsum("bhij,bjhd->bihd", p, v).reshape(B, T, H * hd)


def f16_floor(q, k, v, mask, scale):
    """The reference against itself with its output rounded to f16 (operands are f16-rounded already): the rounding floor of the
    output type, relative to the largest magnitude."""
    want = attention_masked(q, k, v, mask, scale)
    return rel_err(f16(want), want)

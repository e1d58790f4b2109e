"""float64 numpy references of the graph layer's depthwise convolution and of the TinyViT nodes around it (nn.cpp:102-115, mobile-sam.cpp:25-161):
what tests/test_graph_tinyvit_cpu.py takes shapes from and tests/test_gpu_graph_tinyvit.py compares the device against. Maps are [B, H, W, C], depthwise
kernels [k, k, C] (tap-major, as the kernel's operand), tokens [B, T, C]. tests/test_dwconv_ref_cpu.py holds these against the CPU oracle."""
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


def out_extent(n: int, k: int, stride: int, pad: int) -> int:
    return (n + 2 * pad - k) // stride + 1


def depthwise_conv2d(x, w, b=None, stride=1, pad=0):
    """x [B, H, W, C], w [k, k, C], b [C] or None -> [B, OH, OW, C]; taps outside the map are zeros, even kernels like odd ones"""
    x, w = np.asarray(x, np.float64), np.asarray(w, np.float64)
    B, H, W, C = x.shape
    k = w.shape[0]
    assert w.shape == (k, k, C)
    OH, OW = out_extent(H, k, stride, pad), out_extent(W, k, stride, pad)
    xp = np.zeros((B, H + 2 * pad, W + 2 * pad, C))
    xp[:, pad:pad + H, pad:pad + W] = x
    y = np.zeros((B, OH, OW, C))
    for ky in range(k):
        for kx in range(k):
            y += xp[:, ky:ky + (OH - 1) * stride + 1:stride, kx:kx + (OW - 1) * stride + 1:stride] * w[ky, kx]
    return y if b is None else y + np.asarray(b, np.float64)


def kernel_forms(w):
    """the two arrays (numpy order) the weight store can hand over for kernel w [k, k, C]: (kh, kw, 1, C) = ne [C, 1, kw, kh], and (C, kh, kw, 1) = ne [1, kw, kh, C]"""
    w = np.asarray(w)
    return w[:, :, None, :], np.ascontiguousarray(w.transpose(2, 0, 1))[..., None]


def gelu_tanh(x):
    x = np.asarray(x, np.float64)
    return 0.5 * x * (1.0 + np.tanh(np.sqrt(2.0 / np.pi) * x * (1.0 + 0.044715 * x * x)))


def leaky_relu(x, slope):
    x = np.asarray(x, np.float64)
    return np.where(x > 0, x, x * slope)


def conv2d(x, w, b=None, stride=1, pad=0):
    """x [B, H, W, Cin], w [Cout, kh, kw, Cin] -> [B, OH, OW, Cout]"""
    x, w = np.asarray(x, np.float64), np.asarray(w, np.float64)
    B, H, W, _ = x.shape
    co, kh, kw, ci = w.shape
    OH, OW = out_extent(H, kh, stride, pad), out_extent(W, kw, stride, pad)
    xp = np.zeros((B, H + 2 * pad, W + 2 * pad, ci))
    xp[:, pad:pad + H, pad:pad + W] = x
    y = np.zeros((B, OH, OW, co))
    for ky in range(kh):
        for kx in range(kw):
            y += xp[:, ky:ky + (OH - 1) * stride + 1:stride, kx:kx + (OW - 1) * stride + 1:stride] @ w[:, ky, kx].T
    return y if b is None else y + np.asarray(b, np.float64)


def layer_norm(x, w, b, eps=1e-5):
    x = np.asarray(x, np.float64)
    mu = x.mean(-1, keepdims=True)
    var = ((x - mu) ** 2).mean(-1, keepdims=True)
    return (x - mu) / np.sqrt(var + eps) * w + b


def linear(x, w, b=None):
    y = np.asarray(x, np.float64) @ np.asarray(w, np.float64).T
    return y if b is None else y + np.asarray(b, np.float64)


def attention_rel_bias(p, x, heads):
    """x [windows, T, C]; p: norm.weight/bias, qkv.weight/bias (rows per head q | k | v), attention_biases_indexed [heads, T, T], proj.weight/bias"""
    Wn, T, C = x.shape
    hd = C // heads
    qkv = linear(layer_norm(x, p["norm.weight"], p["norm.bias"]), p["qkv.weight"], p["qkv.bias"]).reshape(Wn, T, heads, 3, hd)
    q, k, v = (qkv[:, :, :, i].transpose(0, 2, 1, 3) for i in range(3))  # [windows, heads, T, hd]
    s = q @ k.transpose(0, 1, 3, 2) / np.sqrt(hd) + np.asarray(p["attention_biases_indexed"], np.float64)[None]
    s = np.exp(s - s.max(-1, keepdims=True))
    o = (s / s.sum(-1, keepdims=True)) @ v
    return linear(o.transpose(0, 2, 1, 3).reshape(Wn, T, C), p["proj.weight"], p["proj.bias"])


def window_partition(x, ws):
    """[B, H, W, C] -> ([B * windows, ws * ws, C], padded extent): zero padding at the right and bottom up to whole windows"""
    B, H, W, C = x.shape
    ph, pw = (ws - H % ws) % ws, (ws - W % ws) % ws
    xp = np.zeros((B, H + ph, W + pw, C))
    xp[:, :H, :W] = x
    nh, nw = (H + ph) // ws, (W + pw) // ws
    return xp.reshape(B, nh, ws, nw, ws, C).transpose(0, 1, 3, 2, 4, 5).reshape(B * nh * nw, ws * ws, C), (H + ph, W + pw)


def window_reverse(x, B, H, W, ws, padded):
    Hp, Wp = padded
    nh, nw = Hp // ws, Wp // ws
    return x.reshape(B, nh, nw, ws, ws, -1).transpose(0, 1, 3, 2, 4, 5).reshape(B, Hp, Wp, -1)[:, :H, :W]


def tinyvit_block(p, x, res, heads, ws):
    """x [B, res * res, C]; p: the block's tensors by name below its prefix ('attn.norm.weight', 'local_conv.weight' [3, 3, C], 'local_conv.bias',
    'mlp.fc1.weight', ...) -> [B, res * res, C]  (mobile-sam.cpp:134-161)"""
    B, T, C = x.shape
    assert T == res * res and res != ws
    sub = lambda pre: {k[len(pre):]: v for k, v in p.items() if k.startswith(pre)}
    win, padded = window_partition(np.asarray(x, np.float64).reshape(B, res, res, C), ws)
    att = window_reverse(attention_rel_bias(sub("attn."), win, heads), B, res, res, ws, padded)
    y = att.reshape(B, T, C) + x
    y = depthwise_conv2d(y.reshape(B, res, res, C), p["local_conv.weight"], p["local_conv.bias"], 1, 1).reshape(B, T, C)
    m = sub("mlp.")
    h = gelu_tanh(linear(layer_norm(y, m["norm.weight"], m["norm.bias"]), m["fc1.weight"], m["fc1.bias"]))
    return y + linear(h, m["fc2.weight"], m["fc2.bias"])

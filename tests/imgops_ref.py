"""float64 numpy references for the kernels of csrc/kernels_imgops.hip, in the layouts the launchers take (NHWC; nothing is rounded in here unless a
function says so). tests/test_imgops_ref_cpu.py pins them on torch, on the oracle and on plain numpy; tests/test_gpu_graph_birefnet.py holds the kernels
to them."""
import numpy as np


def f16(a):
    return np.asarray(a, np.float64).astype(np.float16).astype(np.float64)


def sigmoid(x):
    return 1.0 / (1.0 + np.exp(-np.asarray(x, np.float64)))


def _taps(n_in, n_out, dtype):
    """source index pairs and the weight of the second tap along one axis: coordinate o (in - 1) / (out - 1), 0 where out is 1, both taps clamped.
    dtype float32 evaluates the kernel's formula in the kernel's type (the factor rounded, then the product rounded)."""
    o = np.arange(n_out).astype(dtype)
    scale = dtype(n_in - 1) / dtype(n_out - 1) if n_out > 1 else dtype(0)
    s = (o * scale).astype(dtype)
    i0 = np.minimum(s.astype(np.int64), n_in - 1)
    i1 = np.minimum(i0 + 1, n_in - 1)
    return i0, i1, (s - i0.astype(dtype)).astype(dtype)


def image_bilinear_ac(x, oh, ow, dtype=np.float64):
    """vx_image_bilinear_ac_f32: x [B, H, W, C] -> [B, oh, ow, C]; horizontal lerp v0 + (v1 - v0) t, then vertical. dtype = np.float32: the same formula
    with every operation rounded to f32 (no fused multiply-add), the yardstick of the kernel's own rounding."""
    x = np.asarray(x, dtype)
    y0, y1, ty = _taps(x.shape[1], oh, dtype)
    x0, x1, tx = _taps(x.shape[2], ow, dtype)
    ty, tx = ty[None, :, None, None], tx[None, None, :, None]
    r0, r1 = x[:, y0], x[:, y1]
    top = (r0[:, :, x0] + ((r0[:, :, x1] - r0[:, :, x0]).astype(dtype) * tx).astype(dtype)).astype(dtype)
    bot = (r1[:, :, x0] + ((r1[:, :, x1] - r1[:, :, x0]).astype(dtype) * tx).astype(dtype)).astype(dtype)
    return (top + ((bot - top).astype(dtype) * ty).astype(dtype)).astype(dtype)


def image_patches(x, h, w):
    """vx_image_patches_f16 / image_to_patches (birefnet.cpp:153-162): x [B, IH, IW, C] -> [B, h, w, gw gh C]; channel gx + gw (gy + gh c) of pixel (py, px)
    is x[gy h + py, gx w + px, c]. Not rounded."""
    x = np.asarray(x, np.float64)
    B, IH, IW, C = x.shape
    assert IH % h == 0 and IW % w == 0, "Grid must divide image size"
    gh, gw = IH // h, IW // w
    # [B, gy, py, gx, px, c] -> [B, py, px, c, gy, gx]: the channel index is ((c gh) + gy) gw + gx
    return x.reshape(B, gh, h, gw, w, C).transpose(0, 2, 4, 5, 1, 3).reshape(B, h, w, C * gh * gw)


def pixel_gate(p, a, w, bias):
    """vx_pixel_gate_f16: p [rows, C], a [rows, Cg], w [Cg] -> p * f16(sigmoid(bias + a . w)); the gate is rounded to f16, the product is not."""
    g = f16(sigmoid(np.asarray(a, np.float64) @ np.asarray(w, np.float64) + float(bias)))
    return np.asarray(p, np.float64) * g[:, None]


def bilinear_ac(x, oh, ow):
    """vx_bilinear_ac_f16 / vx_bilinear_ac_pix_f16: sf = (out - 1) / (in - 1), or out / in where either side is 1; source o / sf; four weights"""
    x = np.asarray(x, np.float64)

    def axis(n_in, n_out):
        sf = (n_out - 1) / (n_in - 1) if n_out > 1 and n_in > 1 else n_out / n_in
        s = np.arange(n_out) / sf
        i0 = np.clip(np.floor(s).astype(np.int64), 0, n_in - 1)
        return i0, np.clip(i0 + 1, 0, n_in - 1), np.clip(s - i0, 0.0, 1.0)

    y0, y1, fy = axis(x.shape[1], oh)
    x0, x1, fx = axis(x.shape[2], ow)
    fy, fx = fy[None, :, None, None], fx[None, None, :, None]
    r0, r1 = x[:, y0], x[:, y1]
    return r0[:, :, x0] * (1 - fx) * (1 - fy) + r0[:, :, x1] * fx * (1 - fy) + r1[:, :, x0] * (1 - fx) * fy + r1[:, :, x1] * fx * fy


def layer_norm(x, w, b, eps):
    """vx_layernorm_pix_f16: rows [.., C]; the biased variance"""
    x = np.asarray(x, np.float64)
    mean = x.mean(axis=-1, keepdims=True)
    var = ((x - mean) ** 2).mean(axis=-1, keepdims=True)
    return (x - mean) / np.sqrt(var + eps) * np.asarray(w, np.float64) + np.asarray(b, np.float64)


def f16_floor(want):
    """the error of the float64 result rounded to f16, against itself, over its largest value: the floor of any comparison with an f16 output"""
    want = np.asarray(want, np.float64)
    return float(np.abs(f16(want) - want).max() / max(np.abs(want).max(), 1e-30))

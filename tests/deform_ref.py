"""float64 numpy reference for the deformable convolution and the other nodes of a BiRefNet decoder block, on operands already rounded to
f16 (the caller rounds; nothing is rounded in here). Layouts are NHWC; kernels [Cout, kh, kw, Cin]; offsets [B, OH, OW, 2 kh kw] with
channel 2t = dy and 2t + 1 = dx of tap t = ky kw + kx; masks [B, OH, OW, kh kw].

Extension rule of the deformable conv (the oracle's vo_deform_conv2d_nhwc, csrc/kernels_birefnet.hip:103-105): a sample at (py, px) counts
only inside (-1, H) x (-1, W) -- strictly -- and a corner outside the map counts as zero. Positions are formed as f32(integer) + f32(offset)
the way every implementation forms them; the tests plant offsets for which that sum is exact, so floor() is unambiguous."""
import numpy as np


def f16(a):
    return np.asarray(a, np.float64).astype(np.float16).astype(np.float64)


def sigmoid(x):
    return 1.0 / (1.0 + np.exp(-np.asarray(x, np.float64)))


def mean_2d(x):
    """[B, H, W, C] -> [B, 1, 1, C]"""
    return np.asarray(x, np.float64).mean(axis=(1, 2), keepdims=True)


def conv2d(x, w, b=None, pad=0):
    """stride 1; x [B, H, W, Cin], w [Cout, kh, kw, Cin]"""
    x, w = np.asarray(x, np.float64), np.asarray(w, np.float64)
    B, H, W, C = x.shape
    co, kh, kw, _ = w.shape
    xp = np.zeros((B, H + 2 * pad, W + 2 * pad, C))
    xp[:, pad:pad + H, pad:pad + W] = x
    OH, OW = H + 2 * pad - kh + 1, W + 2 * pad - kw + 1
    y = np.zeros((B, OH, OW, co))
    for ky in range(kh):
        for kx in range(kw):
            y += xp[:, ky:ky + OH, kx:kx + OW] @ w[:, ky, kx].T
    return y if b is None else y + np.asarray(b, np.float64)


def deform_sample(x, py, px, with_big=False):
    """x [B, H, W, C]; py, px [B, OH, OW] -> [B, OH, OW, C]: bilinear, zero outside (-1, H) x (-1, W), corners outside the map zero.
    with_big: also the largest magnitude among the corners that count (what an error bound of the blend is linear in)."""
    B, H, W, _ = x.shape
    inside = (py > -1) & (py < H) & (px > -1) & (px < W)
    y0, x0 = np.floor(py).astype(np.int64), np.floor(px).astype(np.int64)
    ly, lx = py - y0, px - x0
    bi = np.arange(B)[:, None, None]
    out = np.zeros(py.shape + (x.shape[3],))
    big = np.zeros_like(out)
    for yy, xx, wgt in ((y0, x0, (1 - ly) * (1 - lx)), (y0, x0 + 1, (1 - ly) * lx), (y0 + 1, x0, ly * (1 - lx)), (y0 + 1, x0 + 1, ly * lx)):
        ok = inside & (yy >= 0) & (yy <= H - 1) & (xx >= 0) & (xx <= W - 1)
        v = x[bi, np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1)]
        out += np.where(ok, wgt, 0.0)[..., None] * v
        big = np.maximum(big, np.where(ok[..., None], np.abs(v), 0.0))
    return (out, big) if with_big else out


def deform_positions(offset, kh, kw, pad):
    """offset [B, OH, OW, 2 kh kw] -> py, px [taps, B, OH, OW] (float64): the f32 sum f32(integer) + f32(offset) every implementation forms"""
    off32 = np.asarray(offset, np.float32)
    OH, OW = off32.shape[1:3]
    oy, ox = np.meshgrid(np.arange(OH), np.arange(OW), indexing="ij")
    py, px = [], []
    for t in range(kh * kw):
        ky, kx = divmod(t, kw)
        py.append(((oy - pad + ky).astype(np.float32)[None] + off32[..., 2 * t]).astype(np.float64))
        px.append(((ox - pad + kx).astype(np.float32)[None] + off32[..., 2 * t + 1]).astype(np.float64))
    return np.stack(py), np.stack(px)


def deform_columns(x, offset, kh, kw, pad, mask=None):
    """The A operand of the deformable conv as a product: -> (cols, big) [B, OH, OW, taps, C], cols = mask * sample, big = |mask| times the
    largest corner magnitude of the sample."""
    x = np.asarray(x, np.float64)
    py, px = deform_positions(offset, kh, kw, pad)
    cols, bigs = [], []
    for t in range(kh * kw):
        s, big = deform_sample(x, py[t], px[t], with_big=True)
        if mask is not None:
            m = np.asarray(mask, np.float64)[..., t:t + 1]
            s, big = s * m, big * np.abs(m)
        cols.append(s)
        bigs.append(big)
    return np.stack(cols, axis=3), np.stack(bigs, axis=3)


def deform_conv2d(x, w, offset, mask=None, pad=0):
    """stride 1, dilation 1, one offset group (nn.cpp:131-148 / torchvision deform_conv2d with the convention above)."""
    w = np.asarray(w, np.float64)
    co, kh, kw, _ = w.shape
    cols, _ = deform_columns(x, offset, kh, kw, pad, mask)
    return cols.reshape(cols.shape[:3] + (-1,)) @ w.reshape(co, -1).T


def bilinear_ac(x, oh, ow):
    """bilinear, align_corners (ggml / vx_bilinear_ac_f16: sf = (out - 1) / (in - 1), or out / in where either side is 1)"""
    x = np.asarray(x, np.float64)
    B, H, W, C = x.shape

    def axis(n_in, n_out):
        sf = (n_out - 1) / (n_in - 1) if n_out > 1 and n_in > 1 else n_out / n_in
        s = np.arange(n_out) / sf
        i0 = np.clip(np.floor(s).astype(np.int64), 0, n_in - 1)
        i1 = np.clip(i0 + 1, 0, n_in - 1)
        return i0, i1, np.clip(s - i0, 0.0, 1.0)

    y0, y1, fy = axis(H, oh)
    x0, x1, fx = axis(W, ow)
    fy, fx = fy[None, :, None, None], fx[None, None, :, None]
    top = x[:, y0][:, :, x0] * (1 - fx) + x[:, y0][:, :, x1] * fx
    bot = x[:, y1][:, :, x0] * (1 - fx) + x[:, y1][:, :, x1] * fx
    return top * (1 - fy) + bot * fy


def _ohwi(w):  # torch OIHW -> [Cout, kh, kw, Cin]
    return np.asarray(w, np.float64).transpose(0, 2, 3, 1)


def aspp_module(sd, prefix, x, pad):
    """aspp_module_deformable (birefnet.cpp:109-114 / visp_oracle.c bf_aspp_module): deformable conv, mul + add, relu"""
    off = conv2d(x, _ohwi(sd[f"{prefix}.conv.offset.weight"]), sd[f"{prefix}.conv.offset.bias"], pad)
    mod = 2.0 * sigmoid(conv2d(x, _ohwi(sd[f"{prefix}.conv.modulator.weight"]), sd[f"{prefix}.conv.modulator.bias"], pad))
    y = deform_conv2d(x, _ohwi(sd[f"{prefix}.conv.conv.weight"]), off, mod, pad)
    return np.maximum(y * np.asarray(sd[f"{prefix}.bn.weight"], np.float64) + np.asarray(sd[f"{prefix}.bn.bias"], np.float64), 0.0)


def decoder_block(sd, prefix, x):
    """basic_decoder_block as bf_decoder_block composes it (visp_oracle.c:2335-2435), in float64 with no intermediate rounding.
    sd: torch-layout tensors (conv kernels OIHW), already rounded to f16; x [B, H, W, Cin]."""
    a = np.maximum(conv2d(x, _ohwi(sd[f"{prefix}.conv_in.weight"]), sd[f"{prefix}.conv_in.bias"], 1), 0.0)
    p = f"{prefix}.dec_att"
    parts = [aspp_module(sd, f"{p}.aspp1", a, 0)] + [aspp_module(sd, f"{p}.aspp_deforms.{i}", a, k // 2) for i, k in enumerate((1, 3, 7))]
    g = np.maximum(conv2d(mean_2d(a), _ohwi(sd[f"{p}.global_avg_pool.1.weight"]), sd[f"{p}.global_avg_pool.1.bias"]), 0.0)
    parts.append(bilinear_ac(g, a.shape[1], a.shape[2]))
    cat = np.concatenate(parts, axis=-1)
    d = np.maximum(conv2d(cat, _ohwi(sd[f"{p}.conv1.weight"]), sd[f"{p}.conv1.bias"]), 0.0)
    return conv2d(d, _ohwi(sd[f"{prefix}.conv_out.weight"]), sd[f"{prefix}.conv_out.bias"], 1)

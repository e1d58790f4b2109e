"""Host restatements of the kernels of the batched MobileSAM decode (csrc/kernels_samprompts.hip), for the GPU suite
tests/test_gpu_sam_prompts_kernels.py to compare with and for tests/test_sam_prompts_ref_cpu.py to pin without a device.

  iou_head(tokens, ws, bs, dtype)  iou_prediction_head: three linears, ReLU behind the first two. float64 is the reference; iou_head_f32_ascending is
                                   numpy's own float32 evaluation with k ascending, whose distance from float64 sizes the kernel's allowance
  choose(iou)                      argmax of the first three predictions, the first index on ties (std::max_element, vision.cpp:80-82)
  i2t(q, k_tok, v_tok, wo, ..)     the image side of a two-way block, K' = LayerNorm(K + out_proj(attention(q, k_tok, v_tok))) and k1' = K' + key_pe, in
                                   float64 throughout: the reference the image-side chain (and the fused kernel that was measured against it) is held to
  process_masks(planes, chosen..)  sam_process_mask per prompt on its chosen plane: the two interpolate passes in the kernel's float32 arithmetic,
                                   operation by operation (no contraction), so the u8 result is the kernel's bit for bit
Plain numpy, nothing from the device side."""
from __future__ import annotations

import numpy as np


def iou_head(tokens: np.ndarray, ws, bs, dtype=np.float64) -> np.ndarray:
    """tokens [P, K0] (the f16 values), ws[l] [N_l, K_l], bs[l] [N_l] -> [P, N_2] in `dtype` (numpy's matmul order)"""
    x = np.asarray(tokens).astype(dtype)
    for l in range(3):
        x = x @ np.asarray(ws[l]).astype(dtype).T + np.asarray(bs[l]).astype(dtype)
        if l < 2:
            x = np.maximum(x, 0)
    return x


def iou_head_f32_ascending(tokens: np.ndarray, ws, bs) -> np.ndarray:
    """the same in float32, every sum one chain with k ascending: acc += w[n][k] * x[k] (product rounded, then the sum), bias last"""
    x = np.asarray(tokens).astype(np.float32)
    for l in range(3):
        w, b = np.asarray(ws[l], np.float32), np.asarray(bs[l], np.float32)
        acc = np.zeros((x.shape[0], w.shape[0]), np.float32)
        for k in range(w.shape[1]):
            acc = acc + x[:, k : k + 1] * w[None, :, k]
        x = acc + b
        if l < 2:
            x = np.maximum(x, np.float32(0))
    return x


def choose(iou: np.ndarray) -> np.ndarray:
    """[P, >= 3] -> int32 [P]: np.argmax returns the first of equal maxima, as std::max_element does"""
    return np.argmax(np.asarray(iou)[:, :3], axis=1).astype(np.int32)


def interpolate(src: np.ndarray, sw: int, sh: int, dw: int, dh: int) -> np.ndarray:
    """sam::interpolate_bilinear (mobile-sam.cpp:485-516) of the top-left sw x sh of src [rows, cols] -> float32 [dh, dw]: half-pixel centres, source
    clamped at 0 and extent - 1, every operation rounded to float32 on its own"""
    f = np.float32
    src = np.asarray(src, f)
    scale_x, scale_y = f(sw) / f(dw), f(sh) / f(dh)
    sx = np.maximum((np.arange(dw, dtype=f) + f(0.5)) * scale_x - f(0.5), f(0))
    sy = np.maximum((np.arange(dh, dtype=f) + f(0.5)) * scale_y - f(0.5), f(0))
    x0, y0 = sx.astype(np.int64), sy.astype(np.int64)
    x1, y1 = np.minimum(x0 + 1, sw - 1), np.minimum(y0 + 1, sh - 1)
    wx, wy = (sx - x0.astype(f))[None, :], (sy - y0.astype(f))[:, None]
    v00, v01 = src[y0][:, x0], src[y0][:, x1]
    v10, v11 = src[y1][:, x0], src[y1][:, x1]
    one = f(1)
    v0 = (one - wx) * v00 + wx * v01
    v1 = (one - wx) * v10 + wx * v11
    return ((one - wy) * v0 + wy * v1).astype(f)


def process_mask(plane: np.ndarray, target_w: int, target_h: int, image_size: int = 1024) -> np.ndarray:
    """sam_process_mask (mobile-sam.cpp:556-583): plane [m, m] -> image_size^2, crop to the scaled extent, resize to the target, threshold -> u8 [h, w]"""
    f = np.float32
    m = plane.shape[0]
    scaled = interpolate(plane, m, m, image_size, image_size)
    up = f(image_size) / f(max(target_w, target_h))
    sw, sh = int(f(target_w) * up + f(0.5)), int(f(target_h) * up + f(0.5))
    return np.where(interpolate(scaled, sw, sh, target_w, target_h) > 0, 255, 0).astype(np.uint8)


def process_masks(planes: np.ndarray, chosen: np.ndarray, target_w: int, target_h: int, image_size: int = 1024) -> np.ndarray:
    """planes [P, n_planes, m, m], chosen [P] -> u8 [P, h, w]; a chosen value outside the planes reads the nearest one, as the kernel clamps it"""
    c = np.clip(np.asarray(chosen), 0, planes.shape[1] - 1)
    return np.stack([process_mask(planes[p, c[p]], target_w, target_h, image_size) for p in range(planes.shape[0])])


def iou_head_cases():
    """The cases of the iou head suite: (id, tokens f16 [P, 256], ws, bs), widths 256 -> 256 -> 256 -> 4 as in the model. `tie`: predictions 0 and 1 are
    the same row and bias, so equal in any summation order, and both above prediction 2: the first index must be chosen. `close`: rows 0 and 1 equal, biases
    1e-4 apart (the near-tie of tests/test_gpu_tinyvit.py)."""
    out = []
    for name, P, seed in (("p1", 1, 1), ("p3", 3, 2), ("tie", 3, 3), ("close", 3, 4)):
        rng = np.random.default_rng(seed)
        tokens = rng.standard_normal((P, 256)).astype(np.float16)
        ws = [(rng.standard_normal((n, k)) / np.sqrt(k)).astype(np.float32) for n, k in ((256, 256), (256, 256), (4, 256))]
        bs = [(0.1 * rng.standard_normal(n)).astype(np.float32) for n in (256, 256, 4)]
        if name in ("tie", "close"):
            ws[2][1] = ws[2][0]
            ws[2][2] = ws[2][0]
            bs[2][1] = bs[2][0] + (np.float32(1e-4) if name == "close" else np.float32(0))
            bs[2][2] = bs[2][0] - np.float32(0.25)
        out.append((name, tokens, ws, bs))
    return out


def i2t(q, k_tok, v_tok, wo, bo, K, ln_w, ln_b, pe=None, heads=8, eps=1e-5):
    """q [B, n, Ci], k_tok, v_tok [B, T, Ci], wo [C, Ci], bo [C], K [B, n, C], ln_w, ln_b [C], pe [n, C] or None -> (K' [B, n, C], k1' or None), float64:
    per head softmax(q k^T / sqrt(hd)) v, out_proj with bias, residual, LayerNorm over the channels (biased variance), then + pe"""
    f = np.float64
    q, k_tok, v_tok, K = (np.asarray(a).astype(f) for a in (q, k_tok, v_tok, K))
    B, n, Ci = q.shape
    hd = Ci // heads
    qh = q.reshape(B, n, heads, hd).transpose(0, 2, 1, 3)
    kh = k_tok.reshape(B, -1, heads, hd).transpose(0, 2, 1, 3)
    vh = v_tok.reshape(B, -1, heads, hd).transpose(0, 2, 1, 3)
    s = qh @ kh.transpose(0, 1, 3, 2) / np.sqrt(f(hd))
    s = np.exp(s - s.max(axis=-1, keepdims=True))
    ao = ((s / s.sum(axis=-1, keepdims=True)) @ vh).transpose(0, 2, 1, 3).reshape(B, n, Ci)
    x = K + ao @ np.asarray(wo).astype(f).T + np.asarray(bo).astype(f)
    mean = x.mean(axis=-1, keepdims=True)
    var = ((x - mean) ** 2).mean(axis=-1, keepdims=True)
    y = (x - mean) / np.sqrt(var + eps) * np.asarray(ln_w).astype(f) + np.asarray(ln_b).astype(f)
    return y, (None if pe is None else y + np.asarray(pe).astype(f))


def i2t_case(B, n_px, Tk, seed):
    """f16 operands of one i2t case with non-trivial norm weights, bias and pe: dict(q, k_tok, v_tok, wo, bo, K, ln_w, ln_b, pe)"""
    rng = np.random.default_rng(seed)
    h = lambda *s: rng.standard_normal(s).astype(np.float16)
    return dict(q=h(B, n_px, 128), k_tok=h(B, Tk, 128), v_tok=h(B, Tk, 128), wo=(rng.standard_normal((256, 128)) / np.sqrt(128)).astype(np.float16),
                bo=(0.2 * rng.standard_normal(256)).astype(np.float32), K=h(B, n_px, 256), ln_w=(1 + 0.3 * rng.standard_normal(256)).astype(np.float32),
                ln_b=(0.2 * rng.standard_normal(256)).astype(np.float32), pe=h(n_px, 256))

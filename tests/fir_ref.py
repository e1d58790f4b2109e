"""float64 numpy references for the graph layer's MI-GAN kernels, on f16-rounded operands: the x2 FIR upsample (zero insertion, 4x4 depthwise FIR at
pad 2, last row and column dropped: upsample_2d of migan.cpp:32-51 with filter_const the tile [[1, 0], [0, 0]]), clamp, add / mul / sub with a plane
operand and lrelu_agc (migan.cpp:17-26). Maps are NHWC ([B, H, W, C]); a FIR is [4, 4, C] (tap row, tap column, channel), the order of the packed
operand [16][C]. tests/test_fir_ref_cpu.py pins these to torch and to tests/migan_ref.py."""
from __future__ import annotations

import numpy as np

from pool_ref import f16, f16_floor, rel_err  # noqa: F401  (f16_floor: the floor of any comparison with an f16 output)

ADD, MUL, SUB = 0, 1, 2


def clamp(x, lo: float, hi: float) -> np.ndarray:
    """ggml_clamp's comparisons: x < lo ? lo : (x > hi ? hi : x); -0.0 stays -0.0"""
    x = np.asarray(x, np.float64)
    return np.where(x < lo, np.float64(lo), np.where(x > hi, np.float64(hi), x))


def lrelu_agc(x, slope: float = 0.2, gain: float = float(np.sqrt(2.0)), clamp_: float = 256.0) -> np.ndarray:
    x = np.asarray(x, np.float64)
    x = np.where(x > 0, x, x * slope) * gain
    return clamp(x, -clamp_, clamp_) if clamp_ else x


def plane_binary(op: int, a, b) -> np.ndarray:
    """a [B, H, W, C] (op) b [H, W]: one value per pixel for every channel and image"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)[None, :, :, None]
    return a + b if op == ADD else (a * b if op == MUL else a - b)


def perturbed_fir(rng, C: int, gain: float = 4.0) -> np.ndarray:
    """synth._migan_fir's filter as [4, 4, C]: setup_filter([1, 3, 3, 1], gain), each channel scaled by 1 +- a few %, so that a channel mix-up shows"""
    f = np.outer([1.0, 3.0, 3.0, 1.0], [1.0, 3.0, 3.0, 1.0])
    f = f / f.sum() * gain
    return f[:, :, None] * (1.0 + 0.05 * rng.standard_normal(C))[None, None, :]


def asymmetric_fir(rng, C: int, gain: float = 4.0) -> np.ndarray:
    """the same [1, 3, 3, 1] outer product as [4, 4, C] with each of the 16 taps of every channel perturbed on its own by 15 .. 25 %, the signs drawn
    at random except that the centre taps differ in sign from their mirror images ((1, 1) from (2, 2), (1, 2) from (2, 1)): f[ky][kx] != f[kx][ky] !=
    f[3 - ky][3 - kx] in every channel, so a kernel that flips, transposes or mispairs its taps shows (the symmetric filter hides all three)"""
    f = np.outer([1.0, 3.0, 3.0, 1.0], [1.0, 3.0, 3.0, 1.0])
    f = f / f.sum() * gain
    sign = rng.choice([-1.0, 1.0], (4, 4, C))
    sign[2, 2], sign[2, 1] = -sign[1, 1], -sign[1, 2]
    return f[:, :, None] * (1.0 + sign * rng.uniform(0.15, 0.25, (4, 4, C)))


def upfirdn2x_raw(x, fir) -> np.ndarray:
    """out[Y, X, c] = sum_{i,j} fir[i, j, c] z[Y + i - 2, X + j - 2, c], z[2a, 2b] = x[a, b], zero elsewhere and outside 2h x 2w"""
    x, fir = np.asarray(x, np.float64), np.asarray(fir, np.float64)
    B, h, w, C = x.shape
    z = np.zeros((B, 2 * h + 4, 2 * w + 4, C))  # 2 pixels of padding on every side (the last row / column of z and the pad behind it are zero anyway)
    z[:, 2:2 + 2 * h:2, 2:2 + 2 * w:2] = x
    out = np.zeros((B, 2 * h, 2 * w, C))
    for i in range(4):
        for j in range(4):
            out += fir[i, j] * z[:, i:i + 2 * h, j:j + 2 * w]
    return out


def upfirdn2x(x, fir, plane=None, res=None, agc=None) -> np.ndarray:
    """the FIR upsample with the kernel's epilogue in its order: + plane [2h, 2w]; agc = (gain, clamp): lrelu 0.2, * gain, clamp; + res [B, 2h, 2w, C]"""
    out = upfirdn2x_raw(x, fir)
    if plane is not None:
        out = out + np.asarray(plane, np.float64)[None, :, :, None]
    if agc is not None:
        out = lrelu_agc(out, 0.2, agc[0], agc[1])
    if res is not None:
        out = out + np.asarray(res, np.float64)
    return out


def clamped_fraction(x, fir, plane, agc) -> float:
    """the share of values the clamp of `agc` acts on: |.| > clamp before it"""
    out = upfirdn2x_raw(x, fir)
    if plane is not None:
        out = out + np.asarray(plane, np.float64)[None, :, :, None]
    return float((np.abs(lrelu_agc(out, 0.2, agc[0], 0.0)) > agc[1]).mean())


def depthwise(x, w, bias, stride: int, pad: int) -> np.ndarray:
    """x [B, H, W, C], w [k, k, C], bias [C] or None: cross-correlation, zeros outside the map, extent (n + 2 pad - k) / stride + 1"""
    x, w = np.asarray(x, np.float64), np.asarray(w, np.float64)
    B, H, W, C = x.shape
    k = w.shape[0]
    OH, OW = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    p = np.zeros((B, H + 2 * pad, W + 2 * pad, C))
    p[:, pad:pad + H, pad:pad + W] = x
    out = np.zeros((B, OH, OW, C))
    for i in range(k):
        for j in range(k):
            out += w[i, j] * p[:, i:i + (OH - 1) * stride + 1:stride, j:j + (OW - 1) * stride + 1:stride]
    return out if bias is None else out + np.asarray(bias, np.float64)

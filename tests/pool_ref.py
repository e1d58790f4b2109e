"""float64 numpy references for the graph layer's pooling, SiLU, softmax, softmax expectation (the DFL decode) and row sums, on f16-rounded operands.
Maps are NHWC ([B, H, W, C]); pooling follows ggml_pool_2d: output extent (n + 2 pad - k) / stride + 1 (floor), padded positions never win a maximum,
average has no padding (the graph layer refuses it). tests/test_pool_ref_cpu.py pins these to torch."""
from __future__ import annotations

import numpy as np

MAX, AVG = 0, 1

# (kind, k, stride, pad, C, H, W, B): a map smaller than its kernel; a channel slice of a wider map into a slice of a wider buffer (the test adds the
# strides); the 2x2 / s1 average of AConv; stride 2 with and without pad; a strip tail (W = 19 against 8 outputs per thread) with C across 8-channel
# groups; the largest kernel
POOL_CASES = [(MAX, 5, 1, 2, 16, 3, 3, 2), (MAX, 5, 1, 2, 24, 7, 11, 1), (AVG, 2, 1, 0, 8, 5, 7, 2), (MAX, 3, 2, 1, 16, 9, 13, 1), (MAX, 2, 2, 0, 8, 6, 6, 1),
              (AVG, 3, 1, 0, 40, 4, 19, 3), (MAX, 13, 1, 6, 8, 4, 6, 1)]


def f16(a) -> np.ndarray:
    """the values an f16 tensor holds, as float64"""
    return np.asarray(a, np.float64).astype(np.float16).astype(np.float64)


def rel_err(got, want) -> float:
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float(np.abs(got - want).max() / max(np.abs(want).max(), 1e-30))


def f16_floor(want) -> float:
    """the error of the float64 result rounded to f16, against itself: the floor of any comparison with an f16 output"""
    with np.errstate(over="ignore"):
        return rel_err(np.asarray(want, np.float64).astype(np.float16), want)


def out_extent(n: int, k: int, stride: int, pad: int) -> int:
    return (n + 2 * pad - k) // stride + 1


def pool2d(x, kind: int, k: int, stride: int, pad: int) -> np.ndarray:
    x = np.asarray(x, np.float64)
    B, H, W, C = x.shape
    OH, OW = out_extent(H, k, stride, pad), out_extent(W, k, stride, pad)
    if OH < 1 or OW < 1:
        raise ValueError("pool2d: the kernel does not fit the input")
    if kind == AVG and pad:
        raise ValueError("pool2d: average pooling with padding is not defined here")
    p = np.full((B, H + 2 * pad, W + 2 * pad, C), -np.inf if kind == MAX else 0.0)
    p[:, pad:pad + H, pad:pad + W] = x
    taps = np.stack([p[:, ky:ky + (OH - 1) * stride + 1:stride, kx:kx + (OW - 1) * stride + 1:stride] for ky in range(k) for kx in range(k)])
    return taps.max(0) if kind == MAX else taps.sum(0) / (k * k)


def silu(x) -> np.ndarray:
    x = np.asarray(x, np.float64)
    with np.errstate(over="ignore"):
        return x / (1.0 + np.exp(-x))


def softmax(x) -> np.ndarray:
    """over the last axis, the row maximum subtracted"""
    x = np.asarray(x, np.float64)
    e = np.exp(x - x.max(-1, keepdims=True))
    return e / e.sum(-1, keepdims=True)


def softmax_expect(x, proj) -> np.ndarray:
    """sum_i softmax(x)_i proj_i over the last axis"""
    return (softmax(x) * np.asarray(proj, np.float64)).sum(-1)


def sum_rows(x) -> np.ndarray:
    return np.asarray(x, np.float64).sum(-1, keepdims=True)

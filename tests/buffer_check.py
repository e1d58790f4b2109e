"""The one comparison of a whole output buffer with a reference's (want, allow, written): what every argument-space GPU suite
(tests/test_gpu_*_matrix.py) asserts of what the device left, and what the CPU twins (tests/test_*_ref_cpu.py) hold their seeded defects
against. Plain numpy, nothing from the device side. tests/test_buffer_check_cpu.py holds this file's own seeded defects.

`ref` is (want, allow, written), float64 / float64 / bool arrays of the buffer's shape, over the WHOLE buffer: the gap columns of a strided
output and the guard behind the last row included. `untouched` is what the buffer held before the call: a scalar (0.0 for a zeroed buffer,
rows_ref.CANARY where zero is an expected value) or an array of the buffer's shape (a buffer the call updates in place). An element with
`written` False must still hold the bits of `untouched` (a -0.0 in a zeroed guard is a stray store); a written one is finite and within its
allowance. No argument exempts an element or a case."""
from __future__ import annotations

import numpy as np

BITS = {2: np.uint16, 4: np.uint32, 8: np.uint64}  # f16 and f32 device buffers; float64 is what an emulation may hand in


def _index(flat, shape):
    """a flat position as the index that addresses it: an int for a 1-d buffer, a tuple otherwise"""
    return int(flat) if len(shape) == 1 else tuple(int(i) for i in np.unravel_index(int(flat), shape))


def violations(got, ref, untouched=0.0) -> dict:
    """-> dict(stray: elements the call must leave alone that no longer hold the bits of `untouched`, first_stray: the index of the first,
    nonfinite: written elements that are not finite, outside: elements with |got - want| > allow (a NaN is outside),
    ratio: the largest error / allowance (0 / 0 = 0, e / 0 = inf, inf for a non-finite element), err: the largest error,
    worst: the index of the largest error - allowance, ratios: error / allowance per element)"""
    want, allow, written = ref
    assert got.shape == want.shape == allow.shape == written.shape and got.dtype in (np.float16, np.float32, np.float64) and written.dtype == bool
    as_bits = BITS[got.dtype.itemsize]
    fill = np.ascontiguousarray(np.broadcast_to(np.asarray(untouched).astype(got.dtype), got.shape))
    stray = (np.ascontiguousarray(got).view(as_bits) != fill.view(as_bits)) & ~written
    nonfinite = ~np.isfinite(got) & written
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        err = np.abs(got.astype(np.float64) - want)
        outside = ~(err <= allow)
        ratios = np.where(allow > 0, err / allow, np.where(err > 0, np.inf, 0.0))
        ratios = np.where(nonfinite | np.isnan(err), np.inf, ratios)
        excess = np.where(np.isnan(err), np.inf, err - allow)
    return dict(stray=int(stray.sum()), first_stray=_index(np.argmax(stray), got.shape), nonfinite=int(nonfinite.sum()), outside=int(outside.sum()),
                ratio=float(ratios.max()), err=float(np.where(np.isnan(err), np.inf, err).max()), worst=_index(np.argmax(excess), got.shape), ratios=ratios)


def rejected(v) -> bool:
    """the verdict: what assert_buffer raises on"""
    return bool(v["stray"] or v["nonfinite"] or v["outside"])


def assert_buffer(got, ref, what, untouched=0.0) -> dict:
    """violations(), asserted: nothing stray, nothing non-finite, nothing outside its allowance, in that order -> the dict"""
    v = violations(got, ref, untouched)
    want, allow, _ = ref
    assert v["stray"] == 0, f"{what}: {v['stray']} elements written that the call must leave alone, the first at {v['first_stray']}"
    assert v["nonfinite"] == 0, f"{what}: {v['nonfinite']} written elements are not finite"
    print(f"{what}: max err {v['err']:.3e}, max err / allowance {v['ratio']:.3f}")
    w = v["worst"]
    assert v["outside"] == 0, f"{what}: {v['outside']} of {got.size} elements outside the allowance; worst at {w}: got {got[w]}, want {want[w]:.6g}, allowance {allow[w]:.3g}"
    return v

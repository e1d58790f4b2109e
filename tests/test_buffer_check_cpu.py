"""No device: tests/buffer_check.py -- the comparison every argument-space GPU suite decides pass or fail with -- against its own seeded
defects, on buffers of 2 rows of 8 in rows of 12 (a gap of 4 columns) plus a guard of 8: f16 and f32, flat and 2-d, under zero fill, canary
fill and array fill. Each defect must be reported under its own key and make assert_buffer raise."""
import numpy as np
import pytest

from buffer_check import assert_buffer, rejected, violations

ROWS, N, LD, GUARD = 2, 8, 12, 8
CANARY = -24000.0
LAYOUTS = [(dt, nd) for dt in (np.float16, np.float32) for nd in (1, 2)]
FILLS = ("zero", "canary", "array")


def _buffer(dtype, ndim, fill="zero"):
    """-> (got as a correct call leaves it, ref, untouched): want = 1 + index / 32 (exact in f16), allowance of 4 f16 ulps of 2; row 0 column
    0 has want 0.5 and allowance 0 (bit equality asked)"""
    size = ROWS * LD + GUARD
    untouched = {"zero": 0.0, "canary": CANARY, "array": (np.arange(size) % 7 - 3.0).astype(dtype)}[fill]
    want = np.broadcast_to(np.asarray(untouched, np.float64), (size,)).copy()
    allow, written = np.zeros(size), np.zeros(size, bool)
    idx = (np.arange(ROWS)[:, None] * LD + np.arange(N)[None, :]).reshape(-1)
    want[idx], allow[idx], written[idx] = 1 + idx / 32, 2.0 ** -8, True
    want[0], allow[0] = 0.5, 0.0
    got = want.astype(dtype)
    shape = (size,) if ndim == 1 else (size // 4, 4)
    if isinstance(untouched, np.ndarray):
        untouched = untouched.reshape(shape)
    return got.reshape(shape), tuple(v.reshape(shape) for v in (want, allow, written)), untouched


def _at(flat, got):
    return flat if got.ndim == 1 else tuple(int(i) for i in np.unravel_index(flat, got.shape))


def _raises(got, ref, untouched, text):
    with pytest.raises(AssertionError, match=text):
        assert_buffer(got, ref, "seeded", untouched)


GAP, IN_GUARD, WRITTEN = N + 1, ROWS * LD + 3, LD + 5  # flat positions: a gap column of row 0, a guard element, a written element of row 1


@pytest.mark.parametrize("dtype,ndim", LAYOUTS)
@pytest.mark.parametrize("fill", FILLS)
def test_a_clean_buffer_passes(dtype, ndim, fill):
    got, ref, untouched = _buffer(dtype, ndim, fill)
    v = assert_buffer(got, ref, "clean", untouched)
    assert not rejected(v) and (v["stray"], v["nonfinite"], v["outside"], v["ratio"], v["err"]) == (0, 0, 0, 0.0, 0.0)
    assert v["ratios"].shape == got.shape and not v["ratios"].any()


@pytest.mark.parametrize("dtype,ndim", LAYOUTS)
@pytest.mark.parametrize("fill", FILLS)
def test_a_store_into_the_guard_is_stray(dtype, ndim, fill):
    got, ref, untouched = _buffer(dtype, ndim, fill)
    got[_at(IN_GUARD, got)] = 1.25
    v = violations(got, ref, untouched)
    assert v["stray"] == 1 and v["first_stray"] == _at(IN_GUARD, got) and v["nonfinite"] == 0 and rejected(v)
    _raises(got, ref, untouched, "1 elements written that the call must leave alone, the first at")


@pytest.mark.parametrize("dtype,ndim", LAYOUTS)
def test_a_negative_zero_in_a_zeroed_gap_column_is_stray(dtype, ndim):
    got, ref, untouched = _buffer(dtype, ndim)
    got[_at(GAP, got)] = -0.0
    v = violations(got, ref, untouched)
    assert (v["stray"], v["first_stray"], v["outside"], v["ratio"]) == (1, _at(GAP, got), 0, 0.0)  # by bits alone: its value is the fill's
    _raises(got, ref, untouched, "must leave alone")


@pytest.mark.parametrize("dtype,ndim", LAYOUTS)
@pytest.mark.parametrize("fill", FILLS)
def test_a_written_element_left_at_the_fill_is_outside_not_stray(dtype, ndim, fill):
    got, ref, untouched = _buffer(dtype, ndim, fill)
    at = _at(WRITTEN, got)
    got[at] = untouched[at] if isinstance(untouched, np.ndarray) else untouched
    v = violations(got, ref, untouched)
    assert (v["stray"], v["nonfinite"], v["outside"], v["worst"]) == (0, 0, 1, at) and v["ratio"] > 1
    _raises(got, ref, untouched, "1 of 32 elements outside the allowance; worst at")


@pytest.mark.parametrize("dtype,ndim", LAYOUTS)
@pytest.mark.parametrize("value", (np.nan, np.inf, -np.inf))
def test_a_non_finite_written_element(dtype, ndim, value):
    got, ref, untouched = _buffer(dtype, ndim)
    got[_at(WRITTEN, got)] = value
    v = violations(got, ref, untouched)
    assert (v["stray"], v["nonfinite"], v["outside"]) == (0, 1, 1) and v["ratio"] == np.inf and v["err"] == np.inf and v["worst"] == _at(WRITTEN, got)
    _raises(got, ref, untouched, "1 written elements are not finite")


@pytest.mark.parametrize("ndim", (1, 2))
def test_one_f16_ulp_beyond_the_allowance_against_exactly_on_it(ndim):
    got, ref, untouched = _buffer(np.float16, ndim)
    at = _at(WRITTEN, got)
    ulp = 2.0 ** -10  # of the values in [1, 2)
    assert ref[1][at] == 4 * ulp
    got[at] = ref[0][at] + 4 * ulp
    v = assert_buffer(got, ref, "on the allowance", untouched)
    assert v["outside"] == 0 and v["ratio"] == 1.0 and v["ratios"][at] == 1.0
    got[at] = ref[0][at] + 5 * ulp
    v = violations(got, ref, untouched)
    assert v["outside"] == 1 and v["ratio"] == 1.25 and v["err"] == 5 * ulp and v["worst"] == at and v["ratios"][at] == 1.25
    _raises(got, ref, untouched, "outside the allowance")


@pytest.mark.parametrize("dtype,ndim", LAYOUTS)
def test_allowance_zero(dtype, ndim):
    got, ref, untouched = _buffer(dtype, ndim)
    at = _at(0, got)
    assert ref[1][at] == 0 and ref[2][at] and got[at] == 0.5
    v = assert_buffer(got, ref, "exact", untouched)
    assert v["ratios"][at] == 0 and v["ratio"] == 0  # 0 / 0 counts as 0, and is not dropped
    got[at] = np.nextafter(got[at], dtype(1))
    v = violations(got, ref, untouched)
    assert (v["stray"], v["nonfinite"], v["outside"], v["worst"]) == (0, 0, 1, at) and v["ratio"] == np.inf and v["ratios"][at] == np.inf
    _raises(got, ref, untouched, "outside the allowance")


def test_worst_is_the_largest_excess_and_the_asserts_come_in_order():
    got, ref, untouched = _buffer(np.float32, 2, "canary")
    got[_at(WRITTEN, got)] += 0.5
    got[_at(WRITTEN + 1, got)] += 0.75
    got[_at(WRITTEN - 2, got)] += 0.25
    v = violations(got, ref, untouched)
    assert v["outside"] == 3 and v["worst"] == _at(WRITTEN + 1, got) and v["err"] == 0.75
    got[_at(WRITTEN + 2, got)] = np.nan
    _raises(got, ref, untouched, "not finite")
    got[_at(IN_GUARD, got)] = 0.0  # zero is no fill here
    _raises(got, ref, untouched, "must leave alone")
    assert violations(got, ref, untouched)["first_stray"] == _at(IN_GUARD, got)

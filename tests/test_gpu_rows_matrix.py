"""-m gpu: the row kernels around the matrix-core kernels -- the LayerNorms of kernels_misc.hip, kernels_tinyvit.hip and kernels_swin.hip, the
two window reverse + residual adds, vx_dwconv3x3_f16, vx_add_gelu_f16, vx_add_rows_f16 -- over their argument space (tests/rows_cases.py)
against the float64 references and the derived per-element allowances of tests/rows_ref.py. Every output buffer starts filled with a canary
(zero is an expected value here) and is compared in full, the gap columns of a strided output and a guard of one block of rows behind the last
row included: an element the call must not write must still hold the canary's bits, everything written is finite and within its allowance,
and the SWIN pad rows hold zero bits. One comparison per buffer (buffer_check.assert_buffer, the one tests/test_rows_ref_cpu.py holds the seeded
defects against), no element and no case exempt."""
import numpy as np
import pytest

import rows_cases as T
import rows_ref as R
from buffer_check import assert_buffer
from visioncpp_amd import _lib as L

pytestmark = pytest.mark.gpu

from gpu_util import Report, api, assert_nothing_launched, dev, device_fixture, empty, ids, ptr, release_fixture, sync  # noqa: E402

# (entry point, data kind) -> largest error / allowance seen; reported, not asserted
REPORT = Report("{launches} launches compared in {seconds:.1f} s; largest |got - want| / allowance per entry point and data kind:",
                lambda key, ratio, count: f"  {key[0]:32s} {key[1]:9s} {ratio:.4f}  ({count} launches)")
ENTRY_POINT = {"ln32": "vx_layernorm_f32_f16", "tv_ln": "vx_layernorm_f16", "swin_ln": "vx_swin_layernorm_f16", "swin_ln_strided": "vx_swin_layernorm_strided_f16",
               "swin_merge": "vx_swin_merge_layernorm_f16", "swin_reverse": "vx_swin_window_reverse_add_f16", "tv_reverse": "vx_window_reverse_add_f16",
               "dwconv": "vx_dwconv3x3_f16", "add_gelu": "vx_add_gelu_f16", "add_rows": "vx_add_rows_f16"}
_device = device_fixture(REPORT)
_release_buffers = release_fixture()


def launch(entry, a, size):
    """One call on a canary-filled output buffer of `size` elements -> the whole buffer"""
    dtype = R.out_dtype(entry, a)
    out = dev(R.canary_buffer(size, dtype))
    f = {k: (ptr(v) if isinstance(v, np.ndarray) else v) for k, v in a.items()}  # the operands as device addresses (None stays NULL)
    f["y"] = out.ptr
    if entry == "swin_ln_strided":
        f["rows"] = a["rows_out"]
    L.vx_check(T.call(api(), entry, f, lambda address: address, eps=a.get("eps", 1e-5)))
    sync()
    return out.to_numpy(dtype, (size,))


def compare(got, ref, key, what, zero_bits=None):
    REPORT.add(key, assert_buffer(got, ref, what, untouched=R.CANARY)["ratio"])
    if zero_bits is not None and zero_bits.any():
        assert not got.view(np.uint16)[zero_bits].any(), f"{what}: pad rows that do not hold zero bits"


def check(case):
    a = T.materialize(case)
    ref = R.evaluate(case["entry"], a, T.guard_of(case, a))
    got = launch(case["entry"], a, ref[0].size)
    f32 = got.dtype == np.float32  # without the rounding to f16 the ratio shows the arithmetic alone: reported on its own
    compare(got, ref, (ENTRY_POINT[case["entry"]] + ("/f32" if f32 else ""), case["kind"]), case["id"], R.zero_bit_elements(case["entry"], a, got.size))


@pytest.mark.parametrize("case", T.group("ln32"), ids=ids(T.group("ln32")))
def test_layernorm_f32_f16(case):
    check(case)


@pytest.mark.parametrize("case", T.group("tv_ln"), ids=ids(T.group("tv_ln")))
def test_layernorm_f16(case):
    check(case)


@pytest.mark.parametrize("case", T.group("swin_ln"), ids=ids(T.group("swin_ln")))
def test_swin_layernorm(case):
    check(case)


@pytest.mark.parametrize("case", T.group("swin_ln_strided"), ids=ids(T.group("swin_ln_strided")))
def test_swin_layernorm_strided(case):
    check(case)


@pytest.mark.parametrize("case", T.group("swin_merge"), ids=ids(T.group("swin_merge")))
def test_swin_merge_layernorm(case):
    check(case)


@pytest.mark.parametrize("case", T.group("swin_reverse"), ids=ids(T.group("swin_reverse")))
def test_swin_window_reverse_add(case):
    check(case)


@pytest.mark.parametrize("case", T.group("tv_reverse"), ids=ids(T.group("tv_reverse")))
def test_window_reverse_add(case):
    check(case)


@pytest.mark.parametrize("case", T.group("dwconv"), ids=ids(T.group("dwconv")))
def test_dwconv3x3(case):
    check(case)


@pytest.mark.parametrize("case", T.group("add_gelu"), ids=ids(T.group("add_gelu")))
def test_add_gelu(case):
    check(case)


@pytest.mark.parametrize("case", T.group("add_rows"), ids=ids(T.group("add_rows")))
def test_add_rows(case):
    check(case)


def test_refusals():
    """every refusal returns 0 with its message, before any launch: the scratch all operands point at stays zero"""
    scratch = empty(T.REFUSAL_SCRATCH_BYTES)
    assert T.run_refusals(api(), scratch.ptr) == T.N_REFUSALS > 90
    assert_nothing_launched(scratch, T.REFUSAL_SCRATCH_BYTES)

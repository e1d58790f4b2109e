"""-m gpu: the row kernels around the matrix-core kernels -- the LayerNorms of kernels_misc.hip, kernels_tinyvit.hip and kernels_swin.hip, the
two window reverse + residual adds, vx_dwconv3x3_f16, vx_add_gelu_f16, vx_add_rows_f16 -- over their argument space (tests/rows_cases.py)
against the float64 references and the derived per-element allowances of tests/rows_ref.py. Every output buffer starts filled with a canary
(zero is an expected value here) and is compared in full, the gap columns of a strided output and a guard of one block of rows behind the last
row included: an element the call must not write must still hold the canary's bits, everything written is finite and within its allowance,
and the SWIN pad rows hold zero bits. One comparison per buffer (rows_ref.violations, the one tests/test_rows_ref_cpu.py holds the seeded
defects against), no element and no case exempt."""
import time
from collections import defaultdict

import numpy as np
import pytest

import rows_cases as T
import rows_ref as R
from visioncpp_amd import _lib as L

pytestmark = pytest.mark.gpu

from gpu_util import api, dev, empty, release, sync  # noqa: E402

RATIO = defaultdict(float)  # (entry point, data kind) -> largest error / allowance seen; reported, not asserted
COUNT = defaultdict(int)
ENTRY_POINT = {"ln32": "vx_layernorm_f32_f16", "tv_ln": "vx_layernorm_f16", "swin_ln": "vx_swin_layernorm_f16", "swin_ln_strided": "vx_swin_layernorm_strided_f16",
               "swin_merge": "vx_swin_merge_layernorm_f16", "swin_reverse": "vx_swin_window_reverse_add_f16", "tv_reverse": "vx_window_reverse_add_f16",
               "dwconv": "vx_dwconv3x3_f16", "add_gelu": "vx_add_gelu_f16", "add_rows": "vx_add_rows_f16"}


@pytest.fixture(scope="module", autouse=True)
def _device():
    assert api().vx_device_count() > 0, "no HIP device visible: the product path has no CPU fallback"
    L.vx_check(api().vx_set_device(0))
    t0 = time.time()
    yield
    print(f"\n{sum(COUNT.values())} launches compared in {time.time() - t0:.1f} s; largest |got - want| / allowance per entry point and data kind:")
    for key, ratio in sorted(RATIO.items()):
        print(f"  {key[0]:32s} {key[1]:9s} {ratio:.4f}  ({COUNT[key]} launches)")


@pytest.fixture(autouse=True)
def _release_buffers():
    yield
    release()


def _ptr(a):
    return None if a is None else dev(np.ascontiguousarray(a)).ptr


def launch(entry, a, size):
    """One call on a canary-filled output buffer of `size` elements -> the whole buffer"""
    dtype = R.out_dtype(entry, a)
    out = dev(R.canary_buffer(size, dtype))
    f = {k: (_ptr(v) if isinstance(v, np.ndarray) else v) for k, v in a.items()}  # the operands as device addresses (None stays NULL)
    f["y"] = out.ptr
    if entry == "swin_ln_strided":
        f["rows"] = a["rows_out"]
    L.vx_check(T.call(api(), entry, f, lambda address: address, eps=a.get("eps", 1e-5)))
    sync()
    return out.to_numpy(dtype, (size,))


def compare(got, ref, key, what, zero_bits=None):
    v = R.violations(got, ref)
    want, allow, written = ref
    assert v["stray"] == 0, f"{what}: {v['stray']} elements written that the call must leave alone, the first at {v['first_stray']}"
    assert v["nonfinite"] == 0, f"{what}: {v['nonfinite']} elements are not finite"
    print(f"{what}: max err {v['err']:.3e}, max err / allowance {v['ratio']:.3f}")
    RATIO[key] = max(RATIO[key], v["ratio"])
    COUNT[key] += 1
    w = v["worst"]
    assert v["outside"] == 0, f"{what}: {v['outside']} of {got.size} elements outside the allowance; worst at {w}: got {got[w]}, want {want[w]:.6g}, allowance {allow[w]:.3g}"
    if zero_bits is not None and zero_bits.any():
        assert not got.view(np.uint16)[zero_bits].any(), f"{what}: pad rows that do not hold zero bits"


def check(case):
    a = T.materialize(case)
    ref = R.evaluate(case["entry"], a, T.guard_of(case, a))
    got = launch(case["entry"], a, ref[0].size)
    f32 = got.dtype == np.float32  # without the rounding to f16 the ratio shows the arithmetic alone: reported on its own
    compare(got, ref, (ENTRY_POINT[case["entry"]] + ("/f32" if f32 else ""), case["kind"]), case["id"], R.zero_bit_elements(case["entry"], a, got.size))


def _ids(cases):
    return [c["id"] for c in cases]


@pytest.mark.parametrize("case", T.group("ln32"), ids=_ids(T.group("ln32")))
def test_layernorm_f32_f16(case):
    check(case)


@pytest.mark.parametrize("case", T.group("tv_ln"), ids=_ids(T.group("tv_ln")))
def test_layernorm_f16(case):
    check(case)


@pytest.mark.parametrize("case", T.group("swin_ln"), ids=_ids(T.group("swin_ln")))
def test_swin_layernorm(case):
    check(case)


@pytest.mark.parametrize("case", T.group("swin_ln_strided"), ids=_ids(T.group("swin_ln_strided")))
def test_swin_layernorm_strided(case):
    check(case)


@pytest.mark.parametrize("case", T.group("swin_merge"), ids=_ids(T.group("swin_merge")))
def test_swin_merge_layernorm(case):
    check(case)


@pytest.mark.parametrize("case", T.group("swin_reverse"), ids=_ids(T.group("swin_reverse")))
def test_swin_window_reverse_add(case):
    check(case)


@pytest.mark.parametrize("case", T.group("tv_reverse"), ids=_ids(T.group("tv_reverse")))
def test_window_reverse_add(case):
    check(case)


@pytest.mark.parametrize("case", T.group("dwconv"), ids=_ids(T.group("dwconv")))
def test_dwconv3x3(case):
    check(case)


@pytest.mark.parametrize("case", T.group("add_gelu"), ids=_ids(T.group("add_gelu")))
def test_add_gelu(case):
    check(case)


@pytest.mark.parametrize("case", T.group("add_rows"), ids=_ids(T.group("add_rows")))
def test_add_rows(case):
    check(case)


def test_refusals():
    """every refusal returns 0 with its message, before any launch: the scratch all operands point at stays zero"""
    scratch = empty(T.REFUSAL_SCRATCH_BYTES)
    assert T.run_refusals(api(), scratch.ptr) == T.N_REFUSALS > 90
    sync()
    assert not scratch.to_numpy(np.uint8, (T.REFUSAL_SCRATCH_BYTES,)).any()  # nothing was launched

"""-m gpu: the sampling and halo matrix-core kernels -- vx_deform_conv_f16, vx_bf_deform_cols_f16, vx_mbconv_dw_pw_f16, vx_conv3x3_f16 -- over
their argument space (tests/sampled_cases.py) against the float64 references and the derived per-element allowances of tests/sampled_ref.py.
Every output buffer starts zeroed and is compared in full, what lies in front of `out` and the guard behind the last row included: an element
the call must not write has allowance 0 and must still hold zero bits (reported on its own). One comparison per buffer, no element and no
case exempt."""
import ctypes as C

import numpy as np
import pytest

import gemm_ref as G
import sampled_cases as T
import sampled_ref as R
from buffer_check import assert_buffer
from visioncpp_amd import _lib as L

pytestmark = pytest.mark.gpu

from gpu_util import Report, api, assert_nothing_launched, dev, device_fixture, empty, ids, ptr, release_fixture, sync  # noqa: E402

# (entry point, data kind) -> largest error / allowance seen; reported, not asserted
REPORT = Report("{launches} launches compared in {seconds:.1f} s; largest |got - want| / allowance per entry point and data kind:",
                lambda key, ratio, count: f"  {key[0]:24s} {key[1]:12s} {ratio:.4f}  ({count} launches)")
ENTRY_POINT = {"deform": "vx_deform_conv_f16", "cols": "vx_bf_deform_cols_f16", "mbconv": "vx_mbconv_dw_pw_f16", "halo": "vx_conv3x3_f16"}
_device = device_fixture(REPORT)
_release_buffers = release_fixture()


def launch(entry, a, n):
    """One call on a zero-initialised output buffer of n elements -> the whole buffer"""
    lib = api()
    if entry == "halo":
        f32 = a["epi"] == G.HEAD_OUT
        out = empty(n * (4 if f32 else 2))
        g = L.GemmArgs()
        for k, v in a.items():
            if k in ("A", "W", "bias", "lambda_", "res1", "res2"):
                v = ptr(v)
            elif k == "A_off":
                continue
            setattr(g, k, v)
        g.out = out.ptr
        assert lib.vx_conv3x3_supported(C.byref(g)) == 1
        L.vx_check(lib.vx_conv3x3_f16(C.byref(g), None))
        sync()
        return out.to_numpy(np.float32 if f32 else np.float16, (n,))
    out = empty(n * 2 + 16)  # (16 bytes more: the shifted `out` of the deform group stays inside)
    if entry == "deform":
        d = L.DeformConvArgs()
        om = dev(a["offset"])
        d.x, d.w, d.offset, d.scale, d.bias = ptr(a["x"]), ptr(a["w"]), om.ptr, ptr(a["scale"]), ptr(a["bias"])
        d.mask = om.ptr + 2 * a["mask_col"] if a["mask_mode"] == 2 else ptr(a["mask"])
        for k in ("B", "H", "W", "Cin", "Cout", "k", "pad", "ld_offset", "ld_mask", "mask_mode", "mask_scale", "relu", "ldo"):
            setattr(d, k, a[k])
        d.out = out.ptr + 2 * a["out_off"]
        assert d.out % 8 == 0 and (a["out_off"] == 0 or d.out % 16 == 8)
        L.vx_check(lib.vx_deform_conv_f16(C.byref(d), None))
    elif entry == "cols":
        L.vx_check(lib.vx_bf_deform_cols_f16(ptr(a["x"]), ptr(a["om"]), a["ldom"], out.ptr, a["B"], a["H"], a["W"], a["C"], a["k"], None))
    else:
        L.vx_check(lib.vx_mbconv_dw_pw_f16(*(ptr(a[k]) for k in ("h", "w2", "b2", "w3", "b3", "x")), out.ptr, a["B"], a["H"], a["W"], R.MB_C, R.MB_CO, None))
    sync()
    return out.to_numpy(np.float16, (n + 8,))[:n]


def check(case):
    a = T.materialize(case)
    ref = R.evaluate(case["entry"], a, T.guard_of(case, a))
    got = launch(case["entry"], a, ref[0].size)
    head = case["entry"] == "halo" and a["epi"] == G.HEAD_OUT  # the f32 head epilogue has an allowance of its own kind: reported on its own
    REPORT.add((ENTRY_POINT[case["entry"]] + ("/head" if head else ""), case["kind"]), assert_buffer(got, ref, case["id"])["ratio"])
    return a, got


@pytest.mark.parametrize("case", T.group("deform"), ids=ids(T.group("deform")))
def test_deform_conv(case):
    check(case)


@pytest.mark.parametrize("case", T.group("cols"), ids=ids(T.group("cols")))
def test_deform_cols(case):
    check(case)


@pytest.mark.parametrize("case", T.group("mbconv"), ids=ids(T.group("mbconv")))
def test_mbconv(case):
    a, got = check(case)
    if case["kind"] == "w3-probe":  # output channel n holds 12 + depthwise channel (37 n + 5) % 256 of its pixel (c / 64 plus the pixel's bit), exactly
        h = a["h"].astype(np.float64)
        np.testing.assert_array_equal(got[:h.size // 4].astype(np.float64).reshape(h.shape[:3] + (R.MB_CO,)), T.W3_PROBE_B2 + h[..., T.w3_probe_column(np.arange(R.MB_CO))])


@pytest.mark.parametrize("case", T.group("halo"), ids=ids(T.group("halo")))
def test_halo_conv(case):
    check(case)


def test_refusals():
    """every refusal returns 0 with its message, before any launch: the scratch all operands point at stays zero"""
    lib = api()
    scratch = empty(T.REFUSAL_SCRATCH_BYTES)
    assert T.run_refusals(lib, scratch.ptr) == len(T.DEFORM_REFUSALS) + len(T.MBCONV_REFUSALS) + len(T.HALO_REFUSALS) + len(T.COLS_REFUSALS) > 70
    assert_nothing_launched(scratch, T.REFUSAL_SCRATCH_BYTES)

"""-m gpu: the Depth-Anything head's matrix-core kernels -- vx_headconv_bil_f16, vx_headconv_wide_bil_f16, vx_rcu_fused_f16 and the unfused
vx_bilinear_ac_f16 -- over their argument space (tests/head_cases.py) against the float64 references and the derived per-element allowances of
tests/head_ref.py. Every output buffer starts zeroed and is compared in full, the guard behind the last image included: an element the call
must not write has allowance 0 and must still hold zero bits (reported on its own). One comparison per buffer, no element exempt.

The walk case runs a 36-tile problem on 8 persistent blocks (vx_headconv_set_block_cap): five tiles per block across image boundaries, the
double buffer's steady state -- and must give the bits of the default grid."""
import ctypes as C

import numpy as np
import pytest

import head_cases as T
import head_ref as R
from buffer_check import assert_buffer
from visioncpp_amd import _lib as L

pytestmark = pytest.mark.gpu

from gpu_util import Report, api, assert_nothing_launched, dev, device_fixture, empty, ids, release_fixture, sync  # noqa: E402

# (entry point, data kind) -> largest error / allowance seen; reported, not asserted
REPORT = Report("{launches} launches compared in {seconds:.1f} s; largest |got - want| / allowance per entry point and data kind:",
                lambda key, ratio, count: f"  {key[0]:26s} {key[1]:9s} {ratio:.3f}  ({count} launches)")


def _uncap():
    api().vx_headconv_set_block_cap(0)


_device = device_fixture(REPORT, reset=_uncap)
_release_buffers = release_fixture(reset=_uncap)


def entry_point(a, entry):
    if entry == "headconv":
        return "vx_headconv_bil_f16" if a["cin"] == 32 else f"vx_headconv_wide_bil_f16/{a['cin']}"
    return {"rcu": "vx_rcu_fused_f16", "bilinear": "vx_bilinear_ac_f16"}[entry]


def launch(entry, a, guard, cap=0):
    """One call on a zero-initialised output buffer with `guard` elements behind the last image -> the whole buffer"""
    lib = api()
    x = dev(a["x"])
    if entry == "headconv":
        n = a["B"] * a["H"] * a["W"] + guard
        out = empty(n * 4)
        ops = (dev(a["wfrag"]).ptr, dev(a["bias"]).ptr, dev(a["w3"]).ptr, a["b3"], a["scale"], out.ptr, a["B"], a["H"], a["W"], a["hs"], a["ws"], None)
        if a["cin"] == 32:
            L.vx_check(lib.vx_headconv_set_block_cap(cap))
            try:
                L.vx_check(lib.vx_headconv_bil_f16(x.ptr, *ops))
                sync()
            finally:
                lib.vx_headconv_set_block_cap(0)
        else:
            L.vx_check(lib.vx_headconv_wide_bil_f16(x.ptr, a["cin"], *ops))
            sync()
        return out.to_numpy(np.float32, (n,))
    if entry == "rcu":
        n = a["B"] * a["H"] * a["W"] * 64 + guard
        out = empty(n * 2)
        d = L.RcuArgs()
        d.x, d.w1, d.w2, d.out, d.B, d.H, d.W = x.ptr, dev(a["w1"]).ptr, dev(a["w2"]).ptr, out.ptr, a["B"], a["H"], a["W"]
        for k in ("b1", "b2", "bp", "res2", "wp"):
            if a.get(k) is not None:
                setattr(d, k, dev(a[k]).ptr)
        L.vx_check(lib.vx_rcu_fused_f16(C.byref(d), None))
    else:
        n = a["B"] * a["OH"] * a["OW"] * a["C"] + guard
        out = empty(n * 2)
        L.vx_check(lib.vx_bilinear_ac_f16(x.ptr, out.ptr, a["B"], a["H"], a["W"], a["C"], a["OH"], a["OW"], None))
    sync()
    return out.to_numpy(np.float16, (n,))


def check(case, cap=0):
    a = T.materialize(case)
    guard = T.guard_of(case, a)
    got = launch(case["entry"], a, guard, cap)
    v = assert_buffer(got, R.evaluate(case["entry"], a, guard), case["id"] + (f" cap {cap}" if cap else ""))
    REPORT.add((entry_point(a, case["entry"]), case["kind"]), v["ratio"])
    return got


HEAD = [c for c in T.group("headconv") if "caps" not in c]
WALKS = [c for c in T.group("headconv") if "caps" in c]


@pytest.mark.parametrize("case", HEAD, ids=ids(HEAD))
def test_headconv(case):
    check(case)


@pytest.mark.parametrize("case", WALKS, ids=ids(WALKS))
def test_headconv_capped_walk_gives_the_default_grid_s_bits(case):
    first = None
    for cap in case["caps"]:
        got = check(case, cap)
        if first is None:
            first = got
        else:
            np.testing.assert_array_equal(first.view(np.uint32), got.view(np.uint32))


@pytest.mark.parametrize("case", T.group("rcu"), ids=ids(T.group("rcu")))
def test_rcu(case):
    check(case)


@pytest.mark.parametrize("case", T.group("bilinear"), ids=ids(T.group("bilinear")))
def test_bilinear(case):
    got = check(case)
    if (case["H"], case["W"]) == (case["OH"], case["OW"]):  # the identity resize: the input's bits
        a = T.materialize(case)
        n = a["B"] * a["H"] * a["W"] * a["C"]
        np.testing.assert_array_equal(got[:n].view(np.uint16), a["x"][:n].view(np.uint16))


BATCH = [dict(c, id=c["id"] + "-b3", B=3) for c in T.all_cases()
         if c["id"] in [f"head-second-tile-cin{cin}-pos" for cin in T.CINS] + ["rcu-{}x{}-rcu+res+proj".format(*T.RCU_FIXED[-1]), "bil-up2-c24"]]


@pytest.mark.parametrize("case", BATCH, ids=ids(BATCH))
def test_batch_position_does_not_show_in_the_bits(case):
    """an image's result at position 2 of B = 3 against the same image alone"""
    assert len(BATCH) == 5
    a = T.materialize(case)
    guard = T.guard_of(case, a)
    three = launch(case["entry"], a, guard)
    one = launch(case["entry"], T.batch_slice(case, a, 2), guard)
    per = (one.size - guard)
    assert three.size == 3 * per + guard
    bits = np.uint32 if three.dtype == np.float32 else np.uint16
    np.testing.assert_array_equal(three[2 * per:3 * per].view(bits), one[:per].view(bits))
    assert three[:per].any() and not one[per:].any()


# ---- the refusals: every one returns 0 with its message, before any launch -----------------------------------------------------------------

def test_refusals():
    lib = api()
    scratch = empty(T.REFUSAL_SCRATCH_BYTES)
    assert T.run_refusals(lib, scratch.ptr) == len(T.HEAD_REFUSALS) + len(T.WIDE_REFUSALS) + len(T.RCU_REFUSALS) + len(T.BIL_REFUSALS) > 40
    assert_nothing_launched(scratch, T.REFUSAL_SCRATCH_BYTES)
    assert lib.vx_headconv_set_block_cap(12) == 0 and b"multiple of 8" in lib.vx_last_error()

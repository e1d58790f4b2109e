"""-m gpu: the image entry and exit kernels -- vx_preprocess_patches, vx_preprocess_f32, vx_write_cls_rows, vx_head_out_f32,
vx_minmax_normalize, vx_f32_to_u8 (kernels_misc.hip), vx_tv_preprocess, vx_sam_interpolate (kernels_tinyvit.hip), vx_bf_preprocess_half,
vx_bf_patches (kernels_birefnet.hip) -- over their argument space (tests/pixel_cases.py) against the float64 references and the derived
per-element allowances of tests/pixel_ref.py. Every output buffer starts filled with a canary (the in-place cls rows with their prior contents)
and is compared in full, a guard of one block behind the last element included: an element the call must not write must still hold its prior
bits, everything written is finite and within its allowance, and what must be +0.0 (pad columns, channels 6..7, a negative pre-activation, the
minimum of every normalised image) holds zero bits. u8 outputs are compared byte for byte, guard included. One comparison per buffer
(buffer_check.assert_buffer, or its u8 twin pixel_ref.assert_u8_buffer; tests/test_pixel_ref_cpu.py holds the seeded defects against both), no
element and no case exempt."""
import numpy as np
import pytest

import pixel_cases as T
import pixel_ref as R
from buffer_check import assert_buffer
from visioncpp_amd import _lib as L

pytestmark = pytest.mark.gpu

from gpu_util import Report, api, assert_nothing_launched, dev, device_fixture, empty, ids, release_fixture, sync  # noqa: E402

# (entry point, data kind) -> largest error / allowance seen; reported, not asserted
REPORT = Report("{launches} launches compared in {seconds:.1f} s; largest |got - want| / allowance per entry point and data kind:",
                lambda key, ratio, count: f"  {key[0]:28s} {key[1]:10s} {ratio:.4f}  ({count} launches)")
_device = device_fixture(REPORT)
_release_buffers = release_fixture()
BITS = {1: np.uint8, 2: np.uint16, 4: np.uint32}
SCRATCH_GUARD = 64  # 32-bit words behind vx_minmax_normalize's 2 B words of scratch


def launch(entry, a, first):
    """One call on the output buffer `first` (canary-filled, or the prior contents) -> the whole buffer as the call left it"""
    out = dev(first)
    f = dict(a)
    if entry in ("patches", "pre32"):
        f.update(rgb=dev(a["rgb"]).ptr, out=out.ptr, mean=T.float3(a["mean"]), inv=T.float3(a["inv"]))
    elif entry == "cls":
        f.update(x=out.ptr, cls=dev(a["cls"]).ptr, pos=dev(a["pos"]).ptr)
    elif entry == "head_out":
        f.update(x=dev(a["x"]).ptr, w=dev(a["w"]).ptr, depth=out.ptr)
    elif entry == "minmax":
        scratch = dev(np.full(2 * a["B"] + SCRATCH_GUARD, R.CANARY, np.float32))
        f.update(depth=dev(a["d"]).ptr, out=out.ptr, minmax=scratch.ptr)
    elif entry == "u8":
        f.update(src=dev(a["src"]).ptr, dst=out.ptr)
    elif entry in ("tvpre", "bfhalf"):
        f.update(rgb=dev(a["rgb"]).ptr, out=out.ptr)
    elif entry == "bfpatches":
        f.update(rgb=dev(a["rgb"]).ptr, out=out.ptr, IH=a["gh"] * a["h"], IW=a["gw"] * a["w"])
    else:
        f.update(src=dev(a["src"]).ptr + a["offset"] * a["src"].itemsize, dst=out.ptr)
    L.vx_check(T.call(api(), entry, f, lambda address: address))
    sync()
    if entry == "minmax":  # the scratch is 2 B words: nothing behind them is written (what the call leaves IN them is unspecified)
        behind = scratch.to_numpy(np.uint32, (2 * a["B"] + SCRATCH_GUARD,))[2 * a["B"]:]
        assert (behind == np.float32(R.CANARY).view(np.uint32)).all(), "a store behind the 2 B words of the min/max scratch"
    return out.to_numpy(first.dtype, first.shape)


def check(case):
    entry = case["entry"]
    a = T.materialize(case)
    guard = T.guard_of(case, a)
    size = R.evaluate(entry, a, guard)[0].size
    first = R.initial_buffer(entry, a, size)
    got = launch(entry, a, first)
    ref = R.evaluate(entry, a, guard, got=got)  # (`got` enters the residue channels alone: their reference is the value minus the STORED hi)
    if got.dtype == np.uint8:
        v = R.assert_u8_buffer(got, ref, case["id"], first)
    else:
        v = assert_buffer(got, ref, case["id"], untouched=first)
    REPORT.add((T.ENTRY_POINT[entry] + ("/u8" if got.dtype == np.uint8 and entry == "sam" else ""), case["kind"]), v["ratio"])
    zero = R.zero_bit_elements(entry, a, size)
    bad = got.view(BITS[got.dtype.itemsize])[zero] != 0
    assert not bad.any(), f"{case['id']}: {int(bad.sum())} elements that must be +0.0 hold other bits, the first at {int(np.flatnonzero(zero)[np.argmax(bad)])}"


@pytest.mark.parametrize("case", T.group("patches"), ids=ids(T.group("patches")))
def test_preprocess_patches(case):
    check(case)


@pytest.mark.parametrize("case", T.group("pre32"), ids=ids(T.group("pre32")))
def test_preprocess_f32(case):
    check(case)


@pytest.mark.parametrize("case", T.group("cls"), ids=ids(T.group("cls")))
def test_write_cls_rows(case):
    check(case)


@pytest.mark.parametrize("case", T.group("head_out"), ids=ids(T.group("head_out")))
def test_head_out_f32(case):
    check(case)


@pytest.mark.parametrize("case", T.group("minmax"), ids=ids(T.group("minmax")))
def test_minmax_normalize(case):
    check(case)


@pytest.mark.parametrize("case", T.group("u8"), ids=ids(T.group("u8")))
def test_f32_to_u8(case):
    check(case)


@pytest.mark.parametrize("case", T.group("tvpre"), ids=ids(T.group("tvpre")))
def test_tv_preprocess(case):
    check(case)


@pytest.mark.parametrize("case", T.group("bfhalf"), ids=ids(T.group("bfhalf")))
def test_bf_preprocess_half(case):
    check(case)


@pytest.mark.parametrize("case", T.group("bfpatches"), ids=ids(T.group("bfpatches")))
def test_bf_patches(case):
    check(case)


@pytest.mark.parametrize("case", T.group("sam"), ids=ids(T.group("sam")))
def test_sam_interpolate(case):
    check(case)


def test_refusals():
    """the base call of every table is accepted; every refusal returns 0 with its message, before any launch: the scratch all operands point
    at stays zero (mean and inv_std, which the launcher itself reads, are host memory)"""
    host = np.zeros(16, np.float32)
    accepted = empty(T.REFUSAL_SCRATCH_BYTES)
    assert T.run_base_calls(api(), accepted.ptr, host.ctypes.data) == 10
    sync()
    scratch = empty(T.REFUSAL_SCRATCH_BYTES)
    assert T.run_refusals(api(), scratch.ptr, host.ctypes.data) == T.N_REFUSALS > 90
    assert_nothing_launched(scratch, T.REFUSAL_SCRATCH_BYTES)
    assert not host.any()

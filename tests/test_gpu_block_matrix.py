"""-m gpu: the token-stationary DINOv2 block kernel vx_dino_block16_f16 over its argument space (tests/block_cases.py) against the float64
reference and the derived per-element allowances of tests/block_ref.py. Every buffer the call is given starts zeroed (x: preloaded, its guard
rows included) and is read back in full: an element the call must not write has allowance 0 and must still hold its initial bits, a written one
is finite and within its allowance. One comparison per buffer, no element exempt. x and cap_x1 are compared against the reference of the inputs;
feat, q, k, v against the reference of the residual stream that came back, so nothing but their own stage's arithmetic is allowed them.

The largest error / allowance per buffer -- split by instance, by row class and, in the hidden-unit probes, by GELU population -- is printed at
module teardown: reported, not asserted (profiles/block16_matrix_ratios.txt holds the numbers a later kernel change is judged against)."""
import ctypes as C

import numpy as np
import pytest

import block_cases as T
import block_ref as R
from buffer_check import assert_buffer
from visioncpp_amd import _lib as L
from visioncpp_amd.vision import DeviceBuffer

pytestmark = pytest.mark.gpu

from gpu_util import Report, api, assert_nothing_launched, dev, device_fixture, empty, release_fixture, sync  # noqa: E402

D, HEADS = R.D, R.HEADS
# (buffer, split) -> largest error / allowance seen
REPORT = Report("{launches} launches compared in {seconds:.1f} s; largest |got - want| / allowance per buffer and split:",
                lambda key, ratio, count: f"  {key[0]:7s} {key[1]:22s} {ratio:.3f}")
_WEIGHTS = {}               # weight set -> its device buffers, uploaded once


def _drop_weights():
    sync()
    _WEIGHTS.clear()


_device = device_fixture(REPORT, reset=_drop_weights)
_release_buffers = release_fixture()


def device_weights(name):
    if name not in _WEIGHTS:
        w = T.weights(name)
        mlp, qkv = T.packed(name, api())
        _WEIGHTS[name] = {k: DeviceBuffer.from_numpy(v) for k, v in dict(w_mlp=mlp, w_qkv=qkv, vec_mlp=w["vec_mlp"], vec_qkv=w["vec_qkv"], vec_tap=w["vec_tap"]).items()}
    return _WEIGHTS[name]


def launch(a, wset):
    """one call on zeroed outputs with their guards, x preloaded -> every buffer the call was given, in full"""
    M, T_ = a["M"], a["T"]
    mlp, qkv, tap = R.flags(a)
    w = device_weights(wset)
    rows = M + R.ROW_GUARD
    xd = dev(np.ascontiguousarray(a["x"], np.float32))
    d = L.DinoBlockArgs()
    d.x, d.M, d.T, d.H, d.q_scale, d.eps = xd.ptr, M, T_, a["H"], a["q_scale"], a["eps"]
    bufs = {"x": (xd, np.float32, (rows, D))}
    if mlp:
        d.att, d.w_mlp, d.vec_mlp = dev(np.ascontiguousarray(a["att"], np.float16)).ptr, w["w_mlp"].ptr, w["vec_mlp"].ptr
        if a["cap"]:
            bufs["cap_x1"] = (empty(rows * D * 4), np.float32, (rows, D))
            d.cap_x1 = bufs["cap_x1"][0].ptr
    if tap:
        bufs["feat"] = (empty(rows * D * 2), np.float16, (rows, D))
        d.feat, d.vec_tap = bufs["feat"][0].ptr, w["vec_tap"].ptr
    if qkv:
        shape = (M // T_ + 1, HEADS, T_, 64)
        for n in "qkv":
            bufs[n] = (empty(int(np.prod(shape)) * 2), np.float16, shape)
        d.q, d.k, d.v, d.w_qkv, d.vec_qkv = bufs["q"][0].ptr, bufs["k"][0].ptr, bufs["v"][0].ptr, w["w_qkv"].ptr, w["vec_qkv"].ptr
    L.vx_check(api().vx_dino_block16_f16(C.byref(d), None))
    sync()
    return {n: b.to_numpy(dt, shape) for n, (b, dt, shape) in bufs.items()}


def per_row(v, M):
    """[rows, 384] or head-major [B + 1, 6, T, 64] -> the largest value of each of the call's M token rows"""
    if v.ndim == 4:
        v = v[:-1].transpose(0, 2, 1, 3).reshape(M, -1)
    return v[:M].max(axis=1)


def compare(name, got, ref, initial, case, splits):
    ratio = assert_buffer(got, ref, f"{case['id']} {name}", untouched=initial)["ratios"]
    for split, mask in splits.items():
        REPORT.add((name, split), float(per_row(ratio, case["M"])[mask].max()) if mask.ndim == 1 else float(ratio[mask].max()), launches=0)


CASES = T.all_cases()


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_block(case):
    a = T.materialize(case)
    M = case["M"]
    got = launch(a, case["wset"])
    ref = R.evaluate(a)
    if R.flags(a)[0]:
        ref.update(R.evaluate(a, x_out=got["x"]))  # feat, q, k, v: of the stream the device wrote
    cls = np.array(T.row_classes(M)) if case["data"] == "mixed" else np.array(["probe"] * M)
    splits = {"inst " + case["inst"]: np.ones(M, bool)}
    splits.update({"rows " + k: cls == k for k in set(cls.tolist())})
    REPORT.launches += 1
    for name in ("x", "cap_x1", "feat", "q", "k", "v"):
        if name not in got:
            continue
        s = dict(splits)
        if name == "x" and "b1" in case:  # the hidden-unit probes: column n of x is hidden unit n + 384 s
            f32 = np.zeros(got["x"].shape, bool)
            f32[:M] = np.isin(np.arange(D) + 384 * case["s"], R.F32_UNITS)
            packed = ~f32
            packed[M:] = False
            s["gelu packed-f16 units"] = packed
            if f32.any():
                s["gelu f32 units"] = f32
        compare(name, got[name], ref[name], a["x"] if name == "x" else 0.0, case, s)
    if case["inst"] == "FTF":
        np.testing.assert_array_equal(got["x"].view(np.uint32), np.ascontiguousarray(a["x"], np.float32).view(np.uint32))
    if case.get("exact_cap"):  # Wo' = I on small integers: x + att bit for bit
        np.testing.assert_array_equal(got["cap_x1"][:M].view(np.uint32), (a["x"][:M] + a["att"][:M].astype(np.float32)).view(np.uint32))


def test_refusals():
    lib = api()
    scratch = empty(T.REFUSAL_SCRATCH_BYTES)
    assert T.run_refusals(lib, scratch.ptr) == len(T.REFUSALS)
    assert_nothing_launched(scratch, T.REFUSAL_SCRATCH_BYTES)

"""-m gpu: the MI-GAN and YOLOv9t stage kernels -- vx_migan_dwconv_f16 (plain and down kernel), vx_migan_upsample_f16, vx_migan_torgb
(kernels_migan.hip), vx_yolo_avgpool2_f16, vx_yolo_spp_f16, vx_yolo_upsample2_f16, vx_yolo_decode (kernels_yolov9t.hip) -- over their argument
space (tests/stage_cases.py) against the float64 references and the derived per-element allowances of tests/stage_ref.py. Every output buffer
starts filled with a canary (vx_yolo_spp_f16's with its input in channels [0, C) of every pixel) and is compared in full, a guard of one block
behind the last element included: an element the call must not write must still hold its prior bits, everything written is finite and within
its allowance. vx_yolo_spp_f16, vx_yolo_upsample2_f16 and the candidate list of vx_yolo_decode are compared bit for bit. One comparison per
buffer (buffer_check.assert_buffer; stage_ref.candidate_faults for the list; tests/test_stage_ref_cpu.py holds the seeded defects against both),
no element and no case exempt. Every FIR case but one per entry runs an asymmetric filter: a kernel that flips, transposes or mispairs its taps
fails here and nowhere else."""
import numpy as np
import pytest

import stage_cases as T
import stage_ref as R
from buffer_check import assert_buffer
from visioncpp_amd import _lib as L

pytestmark = pytest.mark.gpu

from gpu_util import Report, api, assert_nothing_launched, dev, device_fixture, empty, ids, release_fixture, sync  # noqa: E402

# (entry point, data kind) -> largest error / allowance seen; reported, not asserted
REPORT = Report("{launches} launches compared in {seconds:.1f} s; largest |got - want| / allowance per entry point and data kind:",
                lambda key, ratio, count: f"  {key[0]:32s} {key[1]:10s} {ratio:.4f}  ({count} launches)")
_device = device_fixture(REPORT)
_release_buffers = release_fixture()
F32, F16 = np.float32, np.float16


def fir_dev(f):
    """f32 [4, 4, C] -> the packed operand [16][C]"""
    return dev(np.ascontiguousarray(f.reshape(16, -1), F32))


def ptr_of(x):
    return None if x is None else dev(np.ascontiguousarray(x)).ptr


def launch(entry, a, firsts):
    """One call on the output buffers `firsts` {part: canary-filled buffer} -> {part: the whole buffer as the call left it}"""
    outs = {part: dev(first) for part, first in firsts.items()}
    out = outs.get(None)
    if entry in ("dw", "dw_down"):
        f = dict(a, x=ptr_of(a["x"]), w=ptr_of(a["w"].reshape(9, -1)), bias=ptr_of(a["bias"]), fir=fir_dev(a["fir"]).ptr if entry == "dw_down" else None, y=out.ptr)
    elif entry == "up":
        f = dict(a, y=ptr_of(a["y"]), fir=fir_dev(a["fir"]).ptr, noise=ptr_of(a["noise"]), feat=ptr_of(a["feat"]), out=out.ptr)
    elif entry == "torgb":
        f = dict(a, x=ptr_of(a["x"]), w=ptr_of(a["w"]), bias=ptr_of(a["bias"]), prev=ptr_of(a["prev"]), fir=fir_dev(a["fir"]).ptr if a["prev"] is not None else None, img=out.ptr)
    elif entry == "avgpool2":
        f = dict(a, x=ptr_of(a["x"]) + a["c0"] * 2, x_pix=a["pix"], y=out.ptr)
    elif entry == "spp":
        f = dict(a, buf=out.ptr)
    elif entry == "upsample2":
        f = dict(a, x=ptr_of(a["x"]) + a["c0"] * 2, y=out.ptr + a["o0"] * 2)
    else:
        raws = [ptr_of(r) for r in a["raws"]]
        f = dict(a, raw0=raws[0], raw1=raws[1], raw2=raws[2], boxes=outs["boxes"].ptr, scores=outs["scores"].ptr,
                 **{k: outs[k].ptr if a["cand"] else None for k in ("count", "idx", "score")})
    L.vx_check(T.call(api(), entry, f, lambda address: address))
    sync()
    return {part: outs[part].to_numpy(first.dtype, first.shape) for part, first in firsts.items()}


def check(case):
    entry = case["entry"]
    a = T.materialize(case)
    parts = ("boxes", "scores") if entry == "decode" else (None,)
    refs = {part: R.evaluate(entry, a, T.GUARD, part) for part in parts}
    firsts = {part: R.initial_buffer(entry, a, refs[part][0].size, part) for part in parts}
    if entry == "decode" and a["cand"]:
        n = a["B"] * R.n_anchors(a["S"]) * a["nc"]
        count = np.full(a["B"] + T.COUNT_GUARD, R.CANARY_I32, np.int32)
        count[:a["B"]] = 0  # zeroed before the call, as the header requires
        firsts.update(count=count, idx=np.full(n + T.GUARD, R.CANARY_I32, np.int32), score=np.full(n + T.GUARD, R.CANARY, F32))
    got = launch(entry, a, firsts)
    for part in parts:
        v = assert_buffer(got[part], refs[part], case["id"] + ("/" + part if part else ""), untouched=firsts[part])
        REPORT.add((T.ENTRY_POINT[entry] + ("/" + part if part else ""), case["kind"]), v["ratio"])
        if entry in ("spp", "upsample2"):  # bit for bit: a zero keeps its sign
            assert R.bit_faults(got[part], refs[part]) == 0, f"{case['id']}: written elements whose bits are not the source's"
    if entry == "decode" and a["cand"]:
        scores = got["scores"][:-T.GUARD].reshape(a["B"], -1, a["nc"])
        faults = R.candidate_faults(a, scores, got["count"], got["idx"], got["score"], T.GUARD)
        assert not faults, (case["id"], faults)
        stride = scores[0].size
        for b, want in enumerate(R.reference_candidates(a)):  # no class score lies within its allowance of conf: the float64 reference's set too
            assert np.array_equal(np.sort(got["idx"][b * stride:b * stride + got["count"][b]]), want), (case["id"], b)


@pytest.mark.parametrize("case", T.group("dw"), ids=ids(T.group("dw")))
def test_migan_dwconv(case):
    check(case)


@pytest.mark.parametrize("case", T.group("dw_down"), ids=ids(T.group("dw_down")))
def test_migan_dwconv_down(case):
    check(case)


@pytest.mark.parametrize("case", T.group("up"), ids=ids(T.group("up")))
def test_migan_upsample(case):
    check(case)


@pytest.mark.parametrize("case", T.group("torgb"), ids=ids(T.group("torgb")))
def test_migan_torgb(case):
    check(case)


@pytest.mark.parametrize("case", T.group("avgpool2"), ids=ids(T.group("avgpool2")))
def test_yolo_avgpool2(case):
    check(case)


@pytest.mark.parametrize("case", T.group("spp"), ids=ids(T.group("spp")))
def test_yolo_spp(case):
    check(case)


@pytest.mark.parametrize("case", T.group("upsample2"), ids=ids(T.group("upsample2")))
def test_yolo_upsample2(case):
    check(case)


@pytest.mark.parametrize("case", T.group("decode"), ids=ids(T.group("decode")))
def test_yolo_decode(case):
    check(case)


def test_refusals():
    """the base call of every table (and the launchers' other accepted forms) is accepted; every refusal returns 0 with its message, before any
    launch: the scratch all operands point into stays zero. No call is ever launched with a misaligned pointer"""
    accepted = empty(T.REFUSAL_SCRATCH_BYTES)
    assert T.run_base_calls(api(), accepted.ptr) == len(T.REFUSAL_BASES) + len(T.EXTRA_BASES) == 12
    sync()
    scratch = empty(T.REFUSAL_SCRATCH_BYTES)
    assert T.run_refusals(api(), scratch.ptr) == T.N_REFUSALS > 100
    assert_nothing_launched(scratch, T.REFUSAL_SCRATCH_BYTES)

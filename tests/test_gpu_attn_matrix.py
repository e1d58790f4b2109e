"""-m gpu: the five attention entry points over their argument space (tests/attn_cases.py) against the float64 references and the derived
per-element allowance of tests/attn_ref.py. Every output buffer starts zeroed and is compared in full, GUARD_ROWS zeroed rows behind the last row
the call owns included (one full query block, so a store from any row of a tail block lands inside the buffer and is compared): an element the
call must not write has allowance 0 and must still hold zero bits. Nothing here is built to fault; the refusals return before any launch."""
import time
from collections import defaultdict

import numpy as np
import pytest

import attn_cases as T
import attn_ref as R
from buffer_check import assert_buffer
from visioncpp_amd import _lib as L

pytestmark = pytest.mark.gpu

from gpu_util import Report, api, assert_nothing_launched, dev, device_fixture, empty, ids, release_fixture, sync  # noqa: E402

GUARD_ROWS = 256  # the largest query block of the five kernels
WAVE_BITS = {"equal": 0, "compared": 0}
SECONDS = defaultdict(float)  # case group -> wall time of its cases, references included


def _tail():
    return ["wall time per group, float64 references included: " + ", ".join(f"{g} {t:.2f} s" for g, t in SECONDS.items()),
            f"vx_attention_f16, 4 waves against 8 waves: {WAVE_BITS['equal']} of {WAVE_BITS['compared']} outputs bit-identical"]


# (entry point, case group) -> largest error / allowance seen; reported, not asserted
REPORT = Report(f"{len(T.ALL)} cases in {{seconds:.1f}} s; largest |got - want| / allowance per entry point and group:",
                lambda key, ratio, count: f"  {key[0]:34s} {key[1]:10s} {ratio:.3f}", tail=_tail)
_device = device_fixture(REPORT)
_release_buffers = release_fixture()


def _out(want):
    return empty(want.size * 2)


def launch_attention(a, want, waves=0, limit=-1.0):
    out = _out(want)
    try:
        api().vx_attention_set_waves(waves)
        api().vx_attention_set_fast_limit(limit)
        L.vx_check(api().vx_attention_f16(dev(a["q"]).ptr, dev(a["k"]).ptr, dev(a["v"]).ptr, out.ptr, a["B"], a["H"], a["T"], None))
        sync()
    finally:
        api().vx_attention_set_waves(0)
        api().vx_attention_set_fast_limit(-1.0)
    return out.to_numpy(np.float16, want.shape)


def launch_masked(a, want):
    out = _out(want)
    L.vx_check(api().vx_attention_masked_f16(dev(a["q"]).ptr, dev(a["k"]).ptr, dev(a["v"]).ptr, dev(a["mask"]).ptr, out.ptr, a["B"], a["H"], a["T"], a["head_dim"],
                                             a["Hm"], a["Bm"], a["mask_is_f32"], None))
    sync()
    return out.to_numpy(np.float16, want.shape)


def launch_window(a, want):
    """the plain form through vx_window_attention_f16 and its packer, the shifted form through vx_swin_attention_pack_bias and the masked entry point"""
    N, heads = a["N"], a["heads"]
    img = api().vx_window_attention_bias_bytes(N, heads) // 2
    out = _out(want)
    if a["ws"]:
        packed = np.zeros(4 * img, np.uint16)
        L.vx_check(api().vx_swin_attention_pack_bias(a["table"].ctypes.data, a["ws"], heads, packed.ctypes.data))
        L.vx_check(api().vx_window_attention_masked_f16(dev(a["qkv"]).ptr, dev(packed).ptr, out.ptr, a["n_windows"], N, heads, a["nwx"], a["nwy"], None))
    else:
        packed = np.zeros(img, np.uint16)
        bias = np.ascontiguousarray(a["bias"], np.float32)
        L.vx_check(api().vx_window_attention_pack_bias(bias.ctypes.data, N, heads, packed.ctypes.data))
        L.vx_check(api().vx_window_attention_f16(dev(a["qkv"]).ptr, dev(packed).ptr, out.ptr, a["n_windows"], N, heads, None))
    sync()
    return out.to_numpy(np.float16, want.shape)


def launch_small(a, want):
    out = _out(want)
    L.vx_check(api().vx_small_attention_f16(dev(a["q"]).ptr, dev(a["k"]).ptr, dev(a["v"]).ptr, out.ptr, a["Nq"], a["Nk"], a["heads"], a["hd"], None))
    sync()
    return out.to_numpy(np.float16, want.shape)


NAN16 = 0x7E00         # f16 quiet NaN: the 32 rows behind the last token of q, k and v, inside the allocation
FILL32 = 0x7FC5A5A5    # f32 quiet NaN with a payload: what `partial` and its guard hold before a call
PARTIAL_GUARD = 32 * 66 * 2   # floats behind `partial`: two whole part slots of the widest head


def _nan_tail(x):
    """[B, T, H, hd] f16 -> the rows [B * T + 32, H * hd] with 32 rows of NaN behind the last token: a tail key or a clamped query row that leaks is non-finite"""
    rows = x.reshape(-1, x.shape[2] * x.shape[3]).view(np.uint16)
    return np.concatenate([rows, np.full((32, rows.shape[1]), NAN16, np.uint16)])


def launch_cross(a, want, step=None, state=None):
    """One call of vx_attention_cross_f16 (step None) or vx_attention_cross_step_f16 on fresh buffers, or on those of `state` (a former call's).
    -> out [rows + GUARD_ROWS, H * hd] f16, the state. `partial` and its guard are checked after every call that runs step 1."""
    B, H, Tq, Tk, hd = a["B"], a["H"], a["Tq"], a["Tk"], a["head_dim"]
    parts, need = api().vx_attention_cross_parts(Tq, Tk), api().vx_attention_cross_partial_bytes(B, H, Tq, Tk, hd)
    assert parts == T.cross_parts(Tq, Tk) and need == T.cross_partial_bytes(B, H, Tq, Tk, hd)
    if state is None:
        state = dict(q=dev(_nan_tail(a["q"])), k=dev(_nan_tail(a["k"])), v=dev(_nan_tail(a["v"])), out=_out(want),
                     partial=dev(np.full(need // 4 + PARTIAL_GUARD, FILL32, np.uint32)) if need else None)
    part = state["partial"]
    args = (state["q"].ptr, state["k"].ptr, state["v"].ptr, state["out"].ptr, part.ptr if part else None, need, B, H, Tq, Tk, hd, a["scale"], None)
    L.vx_check(api().vx_attention_cross_f16(*args) if step is None else api().vx_attention_cross_step_f16(step, *args))
    sync()
    if part is not None:
        bits = part.to_numpy(np.uint32, (need // 4 + PARTIAL_GUARD,))
        assert (bits[need // 4:] == FILL32).all(), "stores behind vx_attention_cross_partial_bytes"
        slots = bits[:need // 4].reshape(B * H, parts, 32, hd + 2)
        assert np.isfinite(slots[:, :, :Tq].view(np.float32)).all(), "a (m, l, O) row of a live query is not finite, or was not written"
        assert (slots[:, :, Tq:] == FILL32).all(), "a partial row at or beyond T_q was written"
    return state["out"].to_numpy(np.float16, want.shape), state


def check_cross(case, a, ref, key):
    """The fused call twice (the same bits), then the two step calls the lowering makes for a split, against the fused call bit for bit."""
    bits = lambda x: x.view(np.uint16)  # noqa: E731
    got, _ = launch_cross(a, ref[0])
    compare(got, ref, key, case["id"])
    np.testing.assert_array_equal(bits(launch_cross(a, ref[0])[0]), bits(got))
    if T.cross_parts(a["Tq"], a["Tk"]) > 1:
        first, state = launch_cross(a, ref[0], step=1)
        assert not bits(first).any(), "step 1 of a split wrote to out"
        np.testing.assert_array_equal(bits(launch_cross(a, ref[0], step=2, state=state)[0]), bits(got))
    else:
        assert not bits(launch_cross(a, ref[0], step=2)[0]).any(), "step 2 of a single part wrote to out"
        np.testing.assert_array_equal(bits(launch_cross(a, ref[0], step=1)[0]), bits(got))


LAUNCH = {"cross": launch_cross, "attention": launch_attention, "masked": launch_masked, "window": launch_window, "small": launch_small}
ENTRY = {"attention": "vx_attention_f16", "masked": "vx_attention_masked_f16", "window": "vx_window_attention_f16", "shifted": "vx_window_attention_masked_f16",
         "small": "vx_small_attention_f16", "cross": "vx_attention_cross_f16"}


def compare(got, ref, key, what=""):
    REPORT.add(key, assert_buffer(got, ref, what)["ratio"])


def check(case, group):
    t0 = time.perf_counter()
    try:
        _check(case, group)
    finally:
        SECONDS[group] += time.perf_counter() - t0


def _check(case, group):
    a = T.materialize(case)
    ref = R.evaluate(a["entry"], a, GUARD_ROWS)
    key = (ENTRY[group], case.get("data") or case.get("content") or "random")
    if a["entry"] == "cross":
        return check_cross(case, a, ref, key)
    if a["entry"] != "attention":
        compare(LAUNCH[a["entry"]](a, ref[0]), ref, key, case["id"])
        return
    # both block shapes through the hook, and the default rule; from three key tiles on also with every tile on the full path
    for limit in (-1.0, 0.0) if a["T"] > 128 else (-1.0,):
        got = {w: launch_attention(a, ref[0], w, limit) for w in (4, 8, 0)}
        for w, g in got.items():
            compare(g, ref, key, f"{case['id']} waves {w} limit {limit}")
        # the two block shapes walk the same 32-query groups over the same tile stream: the same bits
        WAVE_BITS["compared"] += 1
        WAVE_BITS["equal"] += int(np.array_equal(got[4].view(np.uint16), got[8].view(np.uint16)))
        np.testing.assert_array_equal(got[4].view(np.uint16), got[8].view(np.uint16))
        np.testing.assert_array_equal(got[0].view(np.uint16), got[T.attention_default_waves(a["T"])].view(np.uint16))


@pytest.mark.parametrize("case", T.group("attention"), ids=ids(T.group("attention")))
def test_attention(case):
    check(case, "attention")


@pytest.mark.parametrize("case", T.group("masked"), ids=ids(T.group("masked")))
def test_attention_masked(case):
    check(case, "masked")


@pytest.mark.parametrize("case", T.group("window"), ids=ids(T.group("window")))
def test_window_attention(case):
    check(case, "window")


@pytest.mark.parametrize("case", T.group("shifted"), ids=ids(T.group("shifted")))
def test_window_attention_shifted(case):
    check(case, "shifted")


@pytest.mark.parametrize("case", T.group("small"), ids=ids(T.group("small")))
def test_small_attention(case):
    check(case, "small")


@pytest.mark.parametrize("case", T.group("cross"), ids=ids(T.group("cross")))
def test_attention_cross(case):
    check(case, "cross")


# ---- refusals: 0 and the message, before any launch ------------------------------------------------------------------------------------------

def _refusals(table, base, call):
    scratch = empty(1 << 16)
    for fields, message in table:
        args = dict(base, **fields)
        args = {k: (scratch.ptr + int(v[3:] or 0) if isinstance(v, str) and v.startswith("ptr") else v) for k, v in args.items()}   # "ptr", "ptr+8"
        assert call(args) == 0, f"accepted: {fields}"
        assert message.encode() in api().vx_last_error(), (fields, api().vx_last_error())
    assert_nothing_launched(scratch, 1 << 16)


def test_attention_refusals():
    base = dict(q="ptr", k="ptr", v="ptr", out="ptr", B=1, H=1, T=64)
    _refusals(T.ATTENTION_REFUSALS, base, lambda a: api().vx_attention_f16(a["q"], a["k"], a["v"], a["out"], a["B"], a["H"], a["T"], None))


def test_attention_masked_refusals():
    base = dict(q="ptr", k="ptr", v="ptr", mask="ptr", out="ptr", B=4, H=2, T=32, head_dim=32, Hm=2, Bm=2)
    _refusals(T.MASKED_REFUSALS, base,
              lambda a: api().vx_attention_masked_f16(a["q"], a["k"], a["v"], a["mask"], a["out"], a["B"], a["H"], a["T"], a["head_dim"], a["Hm"], a["Bm"], 0, None))


def test_window_attention_refusals():
    base = dict(qkv="ptr", bias="ptr", out="ptr", n_windows=4, N=49, heads=1, nwx=0, nwy=0)
    _refusals(T.WINDOW_REFUSALS, base,
              lambda a: api().vx_window_attention_masked_f16(a["qkv"], a["bias"], a["out"], a["n_windows"], a["N"], a["heads"], a["nwx"], a["nwy"], None))
    assert api().vx_window_attention_f16(None, None, None, 1, 49, 1, None) == 0 and b"bad operands" in api().vx_last_error()


def test_small_attention_refusals():
    base = dict(q="ptr", k="ptr", v="ptr", out="ptr", Nq=4, Nk=16, heads=1, hd=8)
    _refusals(T.SMALL_REFUSALS, base, lambda a: api().vx_small_attention_f16(a["q"], a["k"], a["v"], a["out"], a["Nq"], a["Nk"], a["heads"], a["hd"], None))


def test_attention_cross_refusals():
    base = dict(step=None, q="ptr", k="ptr", v="ptr", out="ptr", partial="ptr", partial_bytes=1 << 15, B=1, H=2, Tq=7, Tk=7, head_dim=16, scale=0.25)

    def call(a):
        args = (a["q"], a["k"], a["v"], a["out"], a["partial"], a["partial_bytes"], a["B"], a["H"], a["Tq"], a["Tk"], a["head_dim"], a["scale"], None)
        return api().vx_attention_cross_f16(*args) if a["step"] is None else api().vx_attention_cross_step_f16(a["step"], *args)

    _refusals(T.CROSS_REFUSALS, base, call)

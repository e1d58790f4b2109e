"""-m gpu: vx_dconv3x3_f16 over its argument space (tests/dconv_cases.py) against the float64 reference and the derived per-element allowance
of tests/dconv_ref.py. Every output buffer starts zeroed and is compared in full: an element the call must not write (the neighbouring planes,
the slack between cout and out_pix, the guard pixels behind the last image) has allowance 0 and must still hold zero bits.

The stream cases run a 40-tile problem three times: with the launcher's grid capped as on a device with 8 CUs (every persistent block walks five
tiles across tile-shape changes and image boundaries: the next tile's first chunk under the current tile's epilogue, the counted waits with
stores in flight, a tile boundary at every position of the unrolled step loop), with 16 (stride 2), and uncapped (one tile per block)."""
import ctypes as C

import numpy as np
import pytest

import dconv_cases as T
import dconv_ref as R
from buffer_check import assert_buffer
from visioncpp_amd import _lib as L

pytestmark = pytest.mark.gpu

from gpu_util import Report, api, dev, device_fixture, empty, ids, release_fixture, sync  # noqa: E402

# variant -> largest error / allowance seen; reported, not asserted
REPORT = Report("largest |got - want| / allowance per variant:", lambda variant, ratio, count: f"  {variant:13s} {ratio:.3f}")


def _default_grid():
    api().vx_dconv_set_block_cap(0)
    api().vx_dconv_set_resident_mode(-1)


_device = device_fixture(REPORT, reset=_default_grid)
_release_buffers = release_fixture(reset=_default_grid)


def launch(a, cap=0, res_mode=-1, stamps=None):
    """One vx_dconv3x3_f16 call on a zero-initialised output buffer of a["out_size"] elements -> the whole buffer"""
    f32 = a["epi"] != R.DC_F16
    out = empty(a["out_size"] * (4 if f32 else 2))
    d = L.DconvArgs()
    d.x, d.x_plane, d.x_pix = dev(a["x"]).ptr + 2 * a["x_off"], a["x_plane"], a["x_pix"]
    d.cin, d.cout, d.up2, d.B, d.H, d.W = a["cin"], a["cout"], a["up2"], a["B"], a["H"], a["W"]
    d.w = dev(a["w"]).ptr
    d.bias = dev(np.asarray(a["bias"], np.float32)).ptr if a.get("bias") is not None else None
    d.epi, d.act, d.s1, d.s2, d.x_residual, d.a_relu = a["epi"], a["act"], a["s1"], a["s2"], a["x_residual"], a["a_relu"]
    d.bil_hs, d.bil_ws = a["bil_hs"], a["bil_ws"]
    for which in ("res1", "res2"):
        if a.get(which) is not None:
            setattr(d, which, dev(a[which]).ptr + 2 * a[which + "_off"])
            setattr(d, which + "_plane", a[which + "_plane"])
            setattr(d, which + "_pix", a[which + "_pix"])
    d.out, d.out_plane, d.out_pix = out.ptr + (4 if f32 else 2) * a["out_off"], a["out_plane"], a["out_pix"]
    if a["epi"] == R.DC_HEAD_F32:
        d.head_w, d.head_bias, d.head_scale = dev(np.asarray(a["head_w"], np.float32)).ptr, a["head_bias"], a["head_scale"]
    if stamps is not None:
        d.stamps = stamps.ptr
    L.vx_check(api().vx_dconv_set_block_cap(cap))
    api().vx_dconv_set_resident_mode(res_mode)
    try:
        L.vx_check(api().vx_dconv3x3_f16(C.byref(d), None))
        sync()
    finally:
        api().vx_dconv_set_block_cap(0)
        api().vx_dconv_set_resident_mode(-1)
    return out.to_numpy(np.float32 if f32 else np.float16, (a["out_size"],))


def compare(a, got, ref, variant, what=""):
    REPORT.add(variant, assert_buffer(got, tuple(r["out"] for r in ref), what)["ratio"])


def check(case, cap=0):
    a = T.materialize(case)
    mode = case.get("res_mode", -1)
    got = launch(a, cap, mode)
    compare(a, got, R.evaluate(a), T.variant_of(a, mode), case["id"])
    return got


@pytest.mark.parametrize("case", T.group("stream"), ids=ids(T.group("stream")))
def test_stream(case):
    a = T.materialize(case)
    ref = R.evaluate(a)
    mode = case["res_mode"] if "res_mode" in case else -1
    first = None
    for cap in case["caps"]:
        got = launch(a, cap, mode)
        compare(a, got, ref, case["variant"], f"{case['id']} cap {cap}")
        # the same MFMA order per tile whichever block computes it: the grid must not show in the bits
        if first is None:
            first = got
        else:
            np.testing.assert_array_equal(first.view(np.uint16 if got.dtype == np.float16 else np.uint32), got.view(np.uint16 if got.dtype == np.float16 else np.uint32))


@pytest.mark.parametrize("case", T.group("stamps"), ids=ids(T.group("stamps")))
def test_stream_with_stamps(case):
    """The diagnostics instantiation: bit-identical to the product one, and slot 6 of a block's row is the number of (tile, chunk) steps it owns."""
    a = T.materialize(case)
    ref = R.evaluate(a)
    plain = launch(dict(a, stamps=0), 0, case["res_mode"])
    compare(a, plain, ref, T.variant_of(dict(a, stamps=0), case["res_mode"]), f"{case['id']} unstamped")
    tiles = a["B"] * T.tile_count(a["H"], a["W"])
    nch = a["cin"] // 32
    for cap in case["caps"]:
        rows = max(tiles, cap)
        st = empty(rows * 64)
        got = launch(a, cap, case["res_mode"], stamps=st)
        compare(a, got, ref, case["variant"], f"{case['id']} cap {cap}")
        np.testing.assert_array_equal(plain.view(np.uint16), got.view(np.uint16))
        s = st.to_numpy(np.uint64, (rows, 8))
        blocks = T.grid_blocks(tiles, cap) if cap else tiles  # uncapped: any device with at least 40 CUs starts one block per tile
        steps = [len(w) * nch for w in T.block_tiles(tiles, blocks)]
        assert s[:blocks, 6].tolist() == steps, (cap, s[:, 6].tolist())
        assert (s[:blocks, 7] != 0).all() and not s[blocks:].any()


@pytest.mark.parametrize("case", T.group("epilogue"), ids=ids(T.group("epilogue")))
def test_epilogue(case):
    check(case)


@pytest.mark.parametrize("case", T.group("geometry"), ids=ids(T.group("geometry")))
def test_geometry(case):
    check(case)
    if T.tile_count(case["H"], case["W"]) * case["B"] > 8:
        check(case, cap=8)


@pytest.mark.parametrize("case", T.group("padded"), ids=ids(T.group("padded")))
def test_padded_cin(case):
    """NHWC Cin = 48 run as cin = 64 with zero weights: channels 48..63 of a pixel are the next pixel's first 16 (times zero: finite even at
    +-65504) and, for an image's last pixel, past the buffer descriptor (zero-filled, whatever follows: here the next image, then NaNs)."""
    a = T.materialize(case)
    assert np.isnan(a["x"][-64:].astype(np.float32)).all() and a["x_pix"] == 48
    if case["extremes"]:
        assert (np.abs(a["x"][:-64].reshape(-1, 48)[:, :16].astype(np.float32)) == 65504).all()
    check(case)


# ---- the argument contract ----------------------------------------------------------------------------------------------------------------

def _refused(fields, message):
    scratch = empty(1 << 20)
    d = L.DconvArgs()
    d.x = d.w = d.out = d.bias = scratch.ptr
    d.B, d.H, d.W, d.cin, d.cout, d.x_plane, d.out_plane = 1, 16, 32, 64, 64, 16 * 32 * 32, 16 * 32 * 32
    d.epi, d.s1, d.s2 = R.DC_F16, 1.0, 1.0
    for k, v in fields.items():
        setattr(d, k, (scratch.ptr + (v[1] if isinstance(v, tuple) else 0)) if (v == "ptr" or isinstance(v, tuple)) else v)
    assert api().vx_dconv3x3_f16(C.byref(d), None) == 0, f"accepted: {fields}"
    assert message.encode() in api().vx_last_error(), (fields, api().vx_last_error())


XRES = dict(x_residual=1, s1=0.2)
FOLD = "x_residual needs act = 0, no a_relu and an s1"
CONTRACT = [
    (dict(x=0), "null operand"),
    (dict(out=0), "null operand"),
    (dict(cin=48), "Cin 48 must be a multiple of 32"),
    (dict(cin=0), "Cin 0 must be a multiple of 32"),
    (dict(B=0), "empty extent"),
    (dict(out_pix=1 << 20), "pixel indices must fit 32 bits"),
    (dict(B=1 << 16, H=1 << 8, W=1 << 8), "pixel indices must fit 32 bits"),
    (dict(up2=1, H=17), "upsampled extent must be even"),
    (dict(cout=32, H=100, W=100, bil_hs=80, bil_ws=80), "outside the interpolating loader's limits"),
    (dict(cout=64, H=100, W=100, bil_hs=50, bil_ws=50), "outside the interpolating loader's limits"),
    (dict(cout=32, H=100, W=100, bil_hs=50, bil_ws=50, a_relu=1), "outside the interpolating loader's limits"),
    (dict(cout=32, H=100, W=100, bil_hs=50, bil_ws=50, up2=1), "outside the interpolating loader's limits"),
    (dict(cout=32, H=100, W=100, bil_hs=50, bil_ws=50, stamps="ptr"), "outside the interpolating loader's limits"),
    (dict(res2_hs=8, res2_ws=16), "bilinear res2 is not built"),
    (dict(x=("ptr", 8)), "operands must be 16-byte aligned"),
    (dict(out=("ptr", 2)), "operands must be 16-byte aligned"),
    (dict(x_pix=16, cin=32), "pixel strides must be multiples of 8 (input >= 32)"),  # what a 16-channel NHWC map would be
    (dict(x_pix=68), "pixel strides must be multiples of 8 (input >= 32)"),
    (dict(out_pix=68), "pixel strides must be multiples of 8 (input >= 32)"),
    (dict(res1="ptr", res1_pix=36), "pixel strides must be multiples of 8 (input >= 32)"),
    (dict(x_plane=4), "bad input plane stride"),
    (dict(x_plane=16 * 32 * 32 - 8), "bad input plane stride"),
    (dict(x_pix=64, x_plane=16), "bad input plane stride"),
    (dict(x_plane=1 << 30), "input planes span more than 2 GiB"),
    (dict(epi=R.DC_RGB_F32), "the rgb head takes weights padded to 32 outputs"),
    (dict(epi=R.DC_RGB_F32, cout=32, a_relu=1), "the rgb head takes weights padded to 32 outputs"),
    (dict(epi=R.DC_HEAD_F32, cout=32), "the fused depth head is a 32-channel epilogue with head_w set"),
    (dict(epi=R.DC_HEAD_F32, head_w="ptr"), "the fused depth head is a 32-channel epilogue with head_w set"),
    (dict(epi=7), "unknown epilogue 7"),
    (dict(out_plane=36), "plane strides must be multiples of 8"),
    (dict(res2="ptr", res2_plane=12), "plane strides must be multiples of 8"),
    (dict(XRES, cout=32), "x_residual needs cout = 64 <= cin"),
    (dict(XRES, cin=32), "x_residual needs cout = 64 <= cin"),
    (dict(XRES, res1="ptr"), "x_residual needs cout = 64 <= cin"),
    (dict(XRES, up2=1), "x_residual needs cout = 64 <= cin"),
    (dict(XRES, s1=0.0), "x_residual needs cout = 64 <= cin"),
    (dict(cout=48), "Cout 48 not in {32, 64}"),
    # what used to be computed differently from the header, in silence
    (dict(XRES, act=1), FOLD),
    (dict(XRES, act=2), FOLD),
    (dict(XRES, a_relu=1), FOLD),
    (dict(XRES, s1=0.3), FOLD),
    (dict(XRES, s1=1e-6), FOLD),
    (dict(XRES, s1=float("nan")), FOLD),
    (dict(act=3), "unknown activation 3"),
    (dict(epi=R.DC_RGB_F32, cout=32, act=1), "the rgb head has no activation and no residuals"),
    (dict(epi=R.DC_RGB_F32, cout=32, res1="ptr"), "the rgb head has no activation and no residuals"),
    (dict(epi=R.DC_RGB_F32, cout=32, res2="ptr"), "the rgb head has no activation and no residuals"),
    (dict(epi=R.DC_HEAD_F32, cout=32, head_w="ptr", act=2), "the fused depth head applies its own ReLUs and takes no residuals"),
    (dict(epi=R.DC_HEAD_F32, cout=32, head_w="ptr", res1="ptr"), "the fused depth head applies its own ReLUs and takes no residuals"),
    (dict(epi=R.DC_HEAD_F32, cout=32, head_w="ptr", res2="ptr"), "the fused depth head applies its own ReLUs and takes no residuals"),
]


def test_argument_contract():
    """Every VX_REQUIRE of vx_dconv3x3_f16 (and its unknown-Cout error) returns 0 with its message, before any launch; the base call passes them."""
    for fields, message in CONTRACT:
        _refused(fields, message)
    assert api().vx_dconv_set_block_cap(12) == 0 and b"multiple of 8" in api().vx_last_error()
    assert api().vx_dconv_x_residual_supported(0.2, 0, 0) == 1 and api().vx_dconv_x_residual_supported(0.3, 0, 0) == 0

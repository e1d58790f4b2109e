"""-m gpu: vx_gemm_f16 over its argument space (tests/gemm_cases.py) against the float64 reference and the derived per-element allowance of
tests/gemm_ref.py. Every output buffer starts zeroed and is compared in full: an element the call must not write has allowance 0 and
must still hold zero bits (columns >= n_valid, the slack up to ldo, cls rows, dropped window rows, rows beyond M). For the rows beyond M
every buffer carries GUARD_ROWS zeroed rows past the last one the call owns (whole extra images in the scattered layouts): one
tallest block tile, so a store from any row of the tail tile lands inside the buffer and is compared."""
import ctypes as C

import numpy as np
import pytest

import gemm_cases
import gemm_ref as R
from buffer_check import assert_buffer
from visioncpp_amd import _lib as L

pytestmark = pytest.mark.gpu

from gpu_util import Report, api, dev, device_fixture, empty, gemm, ids, release_fixture  # noqa: E402

POINTERS = ("A", "W", "bias", "lambda_", "pos", "res1", "res2", "noise", "out0", "A_off")
GUARD_ROWS = 256  # the tallest block tile
# epilogue -> largest error / allowance seen; reported, not asserted
REPORT = Report("largest |got - want| / allowance per epilogue:", lambda epi, ratio, count: f"  {R.EPI_NAMES[epi]:10s} {ratio:.3f}")
_device = device_fixture(REPORT)
_release_buffers = release_fixture()


class _At:  # a device pointer into a buffer (gpu_util.gemm reads .ptr)
    def __init__(self, buf, byte_off):
        self.buf, self.ptr = buf, buf.ptr + byte_off


def launch(a, want):
    """One vx_gemm_f16 call on zero-initialised outputs, shaped like the arrays of `want` -> {buffer name: array of the whole buffer}."""
    f32 = a["epi"] in R.F32_OUT
    dtype = np.float32 if f32 else np.float16
    bufs = {}
    for name, w in want.items():
        if a["epi"] == R.RESID_F32:  # the stream the call adds to, zero guard rows after it
            x0 = np.zeros(w.shape, np.float32)
            x0[:a["M"]] = a["out0"]
            bufs[name] = dev(x0)
        else:
            bufs[name] = empty(w.size * (4 if f32 else 2))
    kw = {k: v for k, v in a.items() if k not in POINTERS and k not in ("M", "N", "K", "epi", "lda", "ldo")}
    for k in ("lambda_", "pos", "res1", "res2", "noise"):
        if a.get(k) is not None:
            kw[k] = dev(a[k])
    if a["epi"] == R.QKV:
        kw.update(q=bufs["q"], k=bufs["k"], vt=bufs["vt"])
    if a.get("k_splits", 0) > 1:
        kw["k_partial"] = empty(a["k_splits"] * a["M"] * a["N"] * 4)
    abuf = dev(a["A"])
    gemm(_At(abuf, 2 * a.get("A_off", 0)), a["W"], a.get("bias"), a["M"], a["epi"], lda=a.get("lda"), out=bufs.get("out"), ldo=a["ldo"], **kw)
    return {name: b.to_numpy(dtype, want[name].shape) for name, b in bufs.items()}


def check(a):
    want, allow, written = R.evaluate(a, GUARD_ROWS)
    got = launch(a, want)
    for name in want:  # out, or q, k and vt
        REPORT.add(a["epi"], assert_buffer(got[name], (want[name], allow[name], written[name]), name)["ratio"])
    return got


@pytest.mark.parametrize("case", gemm_cases.group("a"), ids=ids(gemm_cases.group("a")))
def test_epilogue_by_tile_form(case):
    check(gemm_cases.materialize(case))


@pytest.mark.parametrize("case", gemm_cases.group("b"), ids=ids(gemm_cases.group("b")))
def test_split_k(case):
    a = gemm_cases.materialize(case)
    first = check(a)
    again = launch(a, first)
    np.testing.assert_array_equal(first["out"].view(np.uint16), again["out"].view(np.uint16))  # the fixed summation order: bit-identical


@pytest.mark.parametrize("case", gemm_cases.group("c"), ids=ids(gemm_cases.group("c")))
def test_conv_geometry(case):
    check(gemm_cases.materialize(case))


def _refused(fields, message):
    scratch = empty(1 << 16)
    g = L.GemmArgs()
    g.A = g.W = g.out = g.bias = scratch.ptr
    g.M, g.N, g.K, g.lda, g.ldo, g.epi = 128, 64, 128, 128, 64, R.F16
    for k, v in fields.items():
        setattr(g, k, scratch.ptr if v == "ptr" else v)
    assert api().vx_gemm_f16(C.byref(g), None) == 0, f"accepted: {fields}"
    assert message.encode() in api().vx_last_error(), (fields, api().vx_last_error())


def test_split_k_refusals():
    sk = dict(K=1280, k_splits=2, k_partial="ptr")
    _refused(dict(sk, k_splits=8), "k_splits = 8 leaves an empty k range for K = 1280")
    supported = "split-K supports the F16, F16_RELU and plain F16_ADD epilogues"
    _refused(dict(sk, epi=R.ADD, res1="ptr", res2="ptr"), supported)
    _refused(dict(sk, epi=R.ADD, res1="ptr", post_gelu=1), supported)
    _refused(dict(sk, epi=R.ADD, res1="ptr", win_ws=7, win_res=7, M=49), supported)
    for epi in (R.GELU, R.RESID_F32, R.TOKENS, R.QKV, R.PIXSHUF, R.HEAD_OUT, R.LRELU_AGC, R.SILU):
        _refused(dict(sk, epi=epi), supported)
    _refused(dict(sk, k_partial=0), "k_partial")
    _refused(dict(sk, n_valid=60), "split-K output columns and row stride must be multiples of 8")


CONV = dict(conv_kh=3, conv_kw=3, conv_stride=1, conv_pad=1, conv_H=8, conv_W=16, conv_Cin=8, conv_OH=8, conv_OW=16)
CONTRACT = [
    (dict(M=0), "empty problem"),
    (dict(K=100), "K=100 must be a multiple of 64"),
    (dict(N=48), "N=48 must be a multiple of 32"),
    (dict(W=0), "null operand"),
    (dict(n_valid=20), "n_valid=20 must be a multiple of 8 for f16 outputs"),
    (dict(ldo=68), "ldo=68 must be a multiple of 8"),
    (dict(epi=R.PIXSHUF, ps_s=2, ps_Cout=12, ps_H=8, ps_W=16, n_valid=48), "pixel-shuffle Cout=12 must be a multiple of 8"),
    (dict(epi=R.QKV, qkv_H=1, qkv_T=64), "QKV epilogue needs N == 3*H*64"),
    (dict(post_gelu=1), "post_gelu needs the F16_ADD epilogue with exactly one residual"),
    (dict(epi=R.ADD, post_gelu=1, res1="ptr", res2="ptr"), "post_gelu needs the F16_ADD epilogue with exactly one residual"),
    (dict(win_ws=7, win_res=7, M=49), "window-order output needs the plain F16_ADD form"),
    (dict(epi=R.ADD, win_ws=7, win_res=7, M=49, K=128, **CONV), "window-order output needs the plain F16_ADD form"),
    (dict(epi=R.ADD, win_ws=7, win_res=9, M=100), "M=100 is not a whole number of 2 x 2 window maps"),
    (dict(epi=R.ADD, win_ws=7, win_res=7, M=49, win_shift=7), "bad window shift / height"),
    (dict(epi=R.LRELU_AGC, noise="ptr"), "lrelu_agc noise plane needs noise_hw > 0"),
    (dict(epi=R.HEAD_OUT, lambda_="ptr"), "head epilogue needs N == 32 and conv3 weights"),
    (dict(epi=R.HEAD_OUT, N=32), "head epilogue needs N == 32 and conv3 weights"),
    (dict(ld_res1=72), "ld_res1=72 needs the SiLU epilogue and a multiple of 8"),
    (dict(epi=R.SILU, ld_res1=68), "ld_res1=68 needs the SiLU epilogue and a multiple of 8"),
    (dict(CONV, conv_Cin=12), "conv Cin=12 must be a multiple of 8"),
    (dict(CONV, conv_pix=4), "conv pixel stride 4 must be a multiple of 8 and >= Cin=8"),
    (dict(CONV, conv_pix=12), "conv pixel stride 12 must be a multiple of 8 and >= Cin=8"),
    (dict(CONV, K=64), "conv K too small"),
    (dict(conv_pix=16), "conv_pix is an implicit-conv field"),
    (dict(lda=132), "lda=132 must be a multiple of 8"),
    (dict(epi=11), "unsupported epilogue 11 (conv=0)"),
    (dict(CONV, epi=R.QKV, qkv_H=1, qkv_T=64, N=192), "unsupported epilogue 5 (conv=1)"),
    (dict(CONV, epi=R.LRELU_AGC), "unsupported epilogue 9 (conv=1)"),
    # the two fields that used to be ignored in silence
    (dict(a_relu=1), "a_relu is an implicit-conv field"),
    (dict(epi=R.RESID_F32, lambda_="ptr", n_valid=32), "n_valid=32 < N=64: the f32 epilogues store all N columns"),
    (dict(epi=R.TOKENS, pos="ptr", tokens_P=16, n_valid=32), "n_valid=32 < N=64: the f32 epilogues store all N columns"),
]


def test_argument_contract():
    """Every VX_REQUIRE of vx_gemm_f16_raw (and the dispatcher's unsupported-epilogue error) returns 0 with its message, before any launch."""
    for fields, message in CONTRACT:
        _refused(fields, message)

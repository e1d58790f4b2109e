"""tests/gemm_ref.py is itself under test here, without a device: the float64 reference against the CPU oracle and the numpy window helper (tests/window_ref.py),
its allowance against a float32 emulation of the kernel (inside) and three seeded corruptions of it (outside), and the case table of
tests/test_gpu_gemm_matrix.py for completeness against the epilogue enum of include/visp_hip_kernels.h."""
import re
from pathlib import Path

import numpy as np
import pytest

import gemm_cases
import gemm_ref as R
from oracle import oracle
from window_ref import windows as _windows

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "visp_hip_kernels.h"


def _f16(rng, *shape, scale=1.0):
    return (rng.standard_normal(shape) * scale).astype(np.float16)


def _plain(rng, M, N, K, epi=R.F16, **kw):
    a = dict(A=_f16(rng, M, K), lda=K, W=_f16(rng, N, K, scale=K ** -0.5), bias=(rng.standard_normal(N) * 0.1).astype(np.float32),
             M=M, N=N, K=K, epi=epi, ldo=N)
    a.update(kw)
    return a


def _close(got, want):  # float32-level agreement with the oracle's f32 arithmetic
    np.testing.assert_allclose(got, want, rtol=2e-5, atol=2e-5 * float(np.abs(want).max()))


@pytest.mark.parametrize("M,N,K", [(77, 96, 128), (131, 64, 64), (300, 128, 192)])
def test_reference_matches_oracle_linear_and_gelu(M, N, K):
    rng = np.random.default_rng(M)
    a = _plain(rng, M, N, K)
    lin = oracle.linear(a["A"].astype(np.float32), a["W"].astype(np.float32), a["bias"])
    _close(R.gemm_ref(a)["out"], lin)
    _close(R.gemm_ref(dict(a, epi=R.RELU))["out"], np.maximum(lin, 0))
    _close(R.gemm_ref(dict(a, epi=R.GELU))["out"], oracle.gelu(lin, oracle.GELU_TANH_F32))
    # row remap: rows 1.. of every group of 51, and a wider lda
    wide = dict(a, A=_f16(rng, (-(-M // 50)) * 51 + 1, K + 8), lda=K + 8, a_group=50, a_group_stride=51, a_row_off=1)
    rows = (np.arange(M) // 50) * 51 + 1 + np.arange(M) % 50
    _close(R.gemm_ref(wide)["out"], oracle.linear(wide["A"].astype(np.float32)[rows, :K], a["W"].astype(np.float32), a["bias"]))


@pytest.mark.parametrize("kh,kw,stride,pad,cin,hw", [(3, 3, 1, 1, 24, (11, 7)), (7, 7, 1, 3, 8, (10, 10)), (1, 1, 2, 0, 64, (11, 7)), (3, 1, 1, 1, 8, (10, 10)),
                                                     (1, 3, 1, 0, 24, (11, 7)), (3, 3, 2, 1, 64, (10, 10))])
def test_reference_matches_oracle_conv(kh, kw, stride, pad, cin, hw):
    rng = np.random.default_rng(kh * 10 + kw)
    B, (H, W), N = 2, hw, 32
    x = _f16(rng, B, H, W, cin + 16)  # the conv reads channels 8 .. 8 + cin of a wider map
    w = _f16(rng, N, kh, kw, cin, scale=(kh * kw * cin) ** -0.5)
    bias = (rng.standard_normal(N) * 0.1).astype(np.float32)
    K = -(-kh * kw * cin // 64) * 64
    wp = _f16(rng, N, K)  # the padding columns of W are not zero: the A operand's padding is
    wp[:, :kh * kw * cin] = w.reshape(N, -1)
    OH, OW = (H + 2 * pad - kh) // stride + 1, (W + 2 * pad - kw) // stride + 1
    a = dict(A=x, A_off=8, conv_pix=cin + 16, W=wp, bias=bias, M=B * OH * OW, N=N, K=K, epi=R.F16, ldo=N, conv_kh=kh, conv_kw=kw, conv_stride=stride,
             conv_pad=pad, conv_H=H, conv_W=W, conv_Cin=cin, conv_OH=OH, conv_OW=OW)
    xs = x[..., 8:8 + cin].astype(np.float32)
    _close(R.gemm_ref(a)["out"].reshape(B, OH, OW, N), oracle.conv2d_nhwc(xs, w.astype(np.float32), bias, stride, pad))
    _close(R.gemm_ref(dict(a, a_relu=1))["out"].reshape(B, OH, OW, N), oracle.conv2d_nhwc(np.maximum(xs, 0), w.astype(np.float32), bias, stride, pad))


@pytest.mark.parametrize("s,c", [(2, 24), (4, 8)])
def test_reference_matches_oracle_conv_transpose(s, c):
    rng = np.random.default_rng(s)
    B, H, W, cin = 2, 5, 7, 64
    x = _f16(rng, B, H, W, cin)
    w = _f16(rng, cin, c, s, s, scale=cin ** -0.5)  # torch [Cin, Cout, kh, kw]
    bias = (rng.standard_normal(c) * 0.1).astype(np.float32)
    N = -(-s * s * c // 32) * 32
    rows = np.zeros((N, cin), np.float16)
    rows[:s * s * c] = w.transpose(2, 3, 1, 0).reshape(s * s * c, cin)
    a = dict(A=x.reshape(-1, cin), lda=cin, W=rows, bias=np.resize(bias, N), M=B * H * W, N=N, K=cin, epi=R.PIXSHUF, ldo=c, n_valid=s * s * c,
             ps_s=s, ps_Cout=c, ps_H=H, ps_W=W)
    _close(R.gemm_ref(a)["out"], oracle.conv_transpose2d_nhwc(x.astype(np.float32), w.astype(np.float32), bias, s))


@pytest.mark.parametrize("shift", [0, 3])
def test_reference_window_order_matches_the_numpy_window_partition(shift):
    """window_reverse(window_partition(y)) = y: an identity product over the window-ordered rows of a map lands every pixel back in place."""
    rng = np.random.default_rng(shift)
    B, H, W, C, ws = 3, 8, 9, 64, 7
    y = _f16(rng, B, H, W, C)
    rows, valid = _windows(y, ws, shift)
    res1 = _f16(rng, B * H * W, C)
    a = dict(A=rows, lda=C, W=np.eye(C, dtype=np.float16), bias=None, M=rows.shape[0], N=C, K=C, epi=R.ADD, ldo=C, res1=res1, win_ws=ws, win_res=W,
             win_res_h=H, win_shift=shift)
    want, _, written = R.evaluate(a)
    np.testing.assert_array_equal(want["out"], y.reshape(-1, C).astype(np.float64) + res1.astype(np.float64))
    assert written["out"].all()
    assert (R.window_pixel_rows(rows.shape[0], ws, W, H, shift) >= 0).tolist() == valid.tolist()


def test_reference_scatter_epilogues_against_plain_numpy():
    rng = np.random.default_rng(1)
    M, K = 333, 64
    a = _plain(rng, M, 384, K, epi=R.QKV, qkv_T=150, qkv_H=2, q_scale=0.125)
    lin = a["A"].astype(np.float64) @ a["W"].astype(np.float64).T + a["bias"]
    want, allow, written = R.evaluate(a)
    full = np.zeros((3 * 150, 3, 2, 64))
    full[:M] = lin.reshape(M, 3, 2, 64)
    full = full.reshape(3, 150, 3, 2, 64)
    np.testing.assert_allclose(want["q"], full[:, :, 0].transpose(0, 2, 1, 3) * 0.125, rtol=1e-12)
    np.testing.assert_allclose(want["vt"], full[:, :, 2].transpose(0, 2, 1, 3), rtol=1e-12)
    assert written["k"].sum() == M * 128 and not written["k"][2, :, 33:].any() and not allow["k"][2, :, 33:].any()
    t = _plain(rng, M, 128, K, epi=R.TOKENS, tokens_P=37, pos=rng.standard_normal((38, 128)).astype(np.float32))
    want, _, written = R.evaluate(t)
    lin = t["A"].astype(np.float64) @ t["W"].astype(np.float64).T + t["bias"]
    assert want["out"].shape == (9 * 38, 128) and not written["out"].reshape(9, 38, 128)[:, 0].any()
    np.testing.assert_allclose(want["out"].reshape(9, 38, 128)[:, 1:].reshape(-1, 128)[:M], lin + np.tile(t["pos"][1:], (9, 1))[:M], rtol=1e-12)


def _emulate(a):
    """what the kernel computes, as numpy float32: f32 product and bias add, one rounding to f16"""
    return (a["A"].astype(np.float32) @ a["W"].astype(np.float32).T + a["bias"]).astype(np.float16)


@pytest.mark.parametrize("K", [64, 192, 1280])
def test_bound_holds_a_float32_emulation_and_rejects_three_corruptions(K):
    rng = np.random.default_rng(K)
    M, N = 200, 64
    a = _plain(rng, M, N, K)
    a["bias"][5] = 3.0  # a loud column next to quiet ones: a maximum-relative tolerance would hide the quiet ones
    want, allow = R.gemm_ref(a)["out"], R.bound(a)["out"]

    def outside(got):
        return np.abs(got.astype(np.float64) - want) > allow

    good = _emulate(a)
    assert not outside(good).any()
    assert allow.max() < 2e-3 * np.abs(want).max(), "the allowance is a per-element quantity far below the old relative tolerance"
    dropped = _emulate(dict(a, A=np.concatenate([a["A"][:, :-8], np.zeros((M, 8), np.float16)], 1)))  # the last 8-wide k chunk
    assert outside(dropped).mean() > 0.9
    shifted = _emulate(dict(a, bias=np.roll(a["bias"], 1)))
    assert outside(shifted).mean() > 0.9
    swapped = good.copy()
    swapped[17] = good[18]
    assert outside(swapped)[17].mean() > 0.9 and not np.delete(outside(swapped), 17, 0).any()
    # ... also when confined to elements of small magnitude: a quiet row (1/64 of the others) with its last chunk dropped
    quiet = dict(a, A=a["A"].copy())
    quiet["A"][40] = (quiet["A"][40].astype(np.float32) / 64).astype(np.float16)
    quiet["bias"] = np.zeros(N, np.float32)
    wq, aq = R.gemm_ref(quiet)["out"], R.bound(quiet)["out"]
    bad = _emulate(quiet)
    assert not (np.abs(bad.astype(np.float64) - wq) > aq).any()
    bad[40] = _emulate(dict(quiet, A=np.concatenate([quiet["A"][:, :-8], np.zeros((M, 8), np.float16)], 1)))[40]
    err = np.abs(bad.astype(np.float64) - wq)
    assert err.max() / np.abs(wq).max() < 4e-3, "the corruption is one the maximum-relative tolerance lets through"
    assert (err > aq)[40].mean() > 0.9


def _header_epilogues():
    body = re.search(r"enum vx_epilogue \{(.*?)\n\};", HEADER.read_text(), re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    found = {name: int(val) for name, val in re.findall(r"\b(VX_EPI_\w+)\s*=\s*(\d+)", body)}
    assert len(found) >= 11, "the header parse found too few epilogues"
    return found


def test_case_table_covers_every_epilogue_on_every_tile_form_and_in_conv_mode():
    epilogues = _header_epilogues()
    assert sorted(epilogues.values()) == list(range(len(R.EPI_NAMES))), "an epilogue the reference does not know"
    assert {f"VX_EPI_{n}": i for i, n in enumerate(R.EPI_NAMES)} == epilogues
    plain = {(c["epi"], c["form"]) for c in gemm_cases.group("a") if c.get("conv_kh", 0) == 0}
    for name, epi in epilogues.items():
        missing = sorted(gemm_cases.forms_of(epi) - {f for e, f in plain if e == epi})
        assert not missing, f"{name} has no plain-mode case on {missing}"
    conv = {c["epi"] for c in gemm_cases.CASES if c.get("conv_kh", 0) > 0 and c.get("k_splits", 0) <= 1}
    assert conv == set(gemm_cases.CONV_EPILOGUES)
    # the dispatcher's tile forms: every `stages` value of dispatch_tile has a form, and the forms claim no other
    src = (ROOT / "vision.cpp_amd" / "csrc" / "kernels_gemm.hip").read_text()
    stages = {int(s) for s in re.findall(r"a\.stages == (\d+)", src)}
    assert stages == {st for st, gran, _ in gemm_cases.FORMS.values() if gran == 128}
    conv_epis = set(re.findall(r"case (VX_EPI_\w+): return (?:dispatch_tile|launch)<[^>]*CONV>", src))
    assert {epilogues[n] for n in conv_epis} == set(gemm_cases.CONV_EPILOGUES)
    # the default dispatcher's own choice between 128 and 192 rows, restated from the slot counts in its formula: the one case that claims
    # the 192x128 form with stages = 0 gets it, every other stages = 0 case on full-width tiles stays on 128x128
    f = re.search(r"c128 = \(\(t128 \+ (\d+)\) / (\d+)\) \* 128, c192 = \(\(t192 \+ (\d+)\) / (\d+)\) \* 192;\s*if \(c192 < c128\)", src)
    assert f, "dispatch_tile no longer chooses by rounds x height: restate its rule here"
    assert [int(x) for x in f.groups()] == [1023, 1024, 767, 768]

    def picks_192(M, N):
        t128, t192 = -(-M // 128) * (N // 128), -(-M // 192) * (N // 128)
        return -(-t192 // 768) * 192 < -(-t128 // 1024) * 128

    auto = [c for c in gemm_cases.CASES if c.get("stages", 0) == 0 and c["N"] % 128 == 0 and c.get("conv_kh", 0) == 0]
    assert {c["id"] for c in auto if picks_192(c["M"], c["N"])} == {"a-f16-dispatcher-picks-192x128"}
    assert {c["id"] for c in auto if c["form"] == "192x128"} == {"a-f16-dispatcher-picks-192x128"}
    # every case is well formed: the form's stages / N granularity, and the tile heights the M of group a is built on
    for c in gemm_cases.CASES:
        st, gran, _ = gemm_cases.FORMS[c["form"]]
        if c["id"].endswith("picks-192x128"):  # stages = 0: the form is the dispatcher's own choice
            continue
        assert c["N"] % gran == 0 and (gran == 128 or c["N"] % (2 * gran) != 0) and c.get("stages", 0) == st, c["id"]

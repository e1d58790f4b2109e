"""No device: the case tables of tests/sampled_cases.py name what they claim, the restated packer and block order agree with the library's host
code, the planted sample positions are what they claim, the references of tests/sampled_ref.py equal the known closed forms, a numpy emulation
of each kernel's arithmetic (its rounding points, in float32 / float16) lies inside the allowance for EVERY case, and modelled wrong kernels lie
outside it for the cases named here. No element and no case is exempt anywhere in this file."""
import re
from collections import defaultdict
from pathlib import Path

import numpy as np
import pytest

import deform_ref as D
import gemm_ref as G
import sampled_cases as T
import sampled_ref as R
from buffer_check import violations
from visioncpp_amd import _lib as L

F32 = np.float32


def f16(x):
    with np.errstate(over="ignore"):
        return np.asarray(x).astype(np.float16).astype(np.float64)


# ---- 1. the tables ----------------------------------------------------------------------------------------------------------------------------

def test_tables_name_what_the_issue_names():
    de = T.group("deform")
    for kind in ("random", "positive"):
        of = [c for c in de if c["kind"] == kind]
        steps = {(T.deform_ck(c["Cin"]), c["Cin"] // T.deform_ck(c["Cin"]) > 1) for c in of}
        assert steps == {(ck, more) for ck in (16, 32, 48, 64) for more in (False, True)}
        assert {c["Cin"] for c in of} >= {16, 80, 32, 160, 48, 96, 64, 128}
        kp = {(c["k"], c["pad"]) for c in of if (c["H"], c["W"]) == (7, 9)}
        assert kp == {(1, 0), (2, 0), (2, 1), (3, 0), (3, 2), (4, 1), (5, 2), (6, 3), (7, 3), (7, 0)}
        extents = {np.sign(T.deform_extent(c)[0] - c["H"]) for c in of if (c["H"], c["W"]) == (7, 9)}
        assert extents == {-1, 0, 1}                                                     # OH below, equal to and above H
        assert any((c["k"], c["pad"], c["H"], c["W"]) == (7, 3, 4, 6) for c in of)       # the kernel larger than the map
        assert {c["Cout"] for c in of if c["k"] == 1 and c["Cin"] == 32} == {8, 32, 40, 128, 136, 256}
        assert {T.deform_m(c) for c in of} >= {9, 33, 64, 65, 70, 192}
        assert any(T.deform_m(c) == 64 and c["B"] == 1 for c in of) and any(T.deform_m(c) == 70 and c["B"] == 2 for c in of)
    assert {c["mask_mode"] for c in de} == {0, 1, 2}
    assert {c["mask_scale"] for c in de if c["mask_mode"] == 2} == {2.0, 1.0, 0.5}
    for c in de:
        a = T.materialize(c)
        assert (a["mask"] is None) == (c["mask_mode"] != 1) and (a["mask_col"] == 2 * c["k"] ** 2) == (c["mask_mode"] == 2)
        if c["mask_mode"] == 1:
            assert a["ld_mask"] == c["k"] ** 2 and a["mask"].shape[1] == a["ld_mask"]
        assert a["w"].shape[0] % 32 == 0 and not a["w"][c["Cout"]:].any()               # the weight image padded to 32 rows with zeros
    assert {c["epi"] for c in de} == {"", "s", "b", "r", "sbr"} == {c["epi"] for c in de if c["kind"] == "positive"}
    ld = {}
    for c in de:
        a, taps = T.materialize(c), c["k"] ** 2
        ld.setdefault(c["ld_offset"], set()).add(a["ld_offset"] - (3 if c["mask_mode"] == 2 else 2) * taps)
        assert a["ld_offset"] >= 2 * taps
    assert ld["exact"] == {0} and all(a["ld_offset"] % 2 for a in (T.materialize(c) for c in de if c["ld_offset"] == "odd")) and 0 not in ld["odd"]
    assert any(T.materialize(c)["ld_offset"] == 2 * c["k"] ** 2 + 1 for c in de if c["ld_offset"] == "odd")
    assert {(c["ldo"], c["out_off"]) for c in de} == {(0, 0), (4, 4), (8, 0)}
    assert {c["kind"] for c in de} == {"random", "positive", "zero-offset", "impulse", "far"}
    assert {(c["tap"], c["corner"]) for c in de if c["kind"] == "impulse"} == {(t, k) for t in range(9) for k in range(4)}
    for c in de:
        if c["kind"] == "far":
            off = np.abs(T.materialize(c)["offset"][:, :2 * c["k"] ** 2].astype(np.float64))
            assert off.min() >= 100 and off.max() <= 2000
    co = T.group("cols")
    assert {(c["C"], c["k"], c["ldom"]) for c in co if c["kind"] == "random"} == {(C, k, ld) for C in (8, 24, 64) for k in (1, 3, 7) for ld in ("exact", "pad8")}
    assert {c["kind"] for c in co} == {"random", "positive", "impulse"}
    assert {T.materialize(c)["ldom"] for c in co if c["k"] == 3} == {27, 32}
    mb = T.group("mbconv")
    for kind in ("random", "positive"):
        assert sorted(T.mbconv_blocks(c) for c in mb if c["kind"] == kind and not c.get("zero_bias")) == [1, 2, 6, 9, 15, 16, 30]
    assert {(c["B"], c["H"], c["W"]) for c in mb} >= {(1, 1, 64), (1, 2, 64), (2, 3, 64), (1, 9, 64), (3, 5, 64), (1, 8, 128), (2, 5, 192)}
    assert {c["tap"] for c in mb if c["kind"] == "impulse"} == set(range(9)) and {c["kind"] for c in mb} == {"random", "positive", "impulse", "w3-probe"}
    assert T.MB_IMPULSE_AT[0][1] == 64 and T.MB_IMPULSE_AT[1][1] % 8 == 0 and T.MB_IMPULSE["W"] > 64  # next to the segment seam, next to a strip seam
    zb = T.materialize(T.case("mbconv-zero-bias"))
    assert not zb["b2"].any() and not zb["b3"].any()
    for c in mb:  # the XCD-aware block order is a permutation for every block count in the table, with q = 0, with nwg % 8 == 0 and without
        nwg = T.mbconv_blocks(c)
        assert sorted(R.mbconv_block(np.arange(nwg), nwg).tolist()) == list(range(nwg)), c["id"]
    assert {T.mbconv_blocks(c) < 8 for c in mb} == {True, False} and any(T.mbconv_blocks(c) % 8 == 0 for c in mb)
    assert all(sorted(R.mbconv_block(np.arange(n), n).tolist()) == list(range(n)) for n in range(1, 200))
    ha = T.group("halo")
    full = {(cin, cout, hw, e) for cin in (32, 64) for cout in (32, 64) for hw in T.HALO_MAPS for e in T.HALO_EPILOGUES if e != "head" or cout == 32}
    assert {(c["cin"], c["cout"], (c["H"], c["W"]), c["epi"]) for c in ha if c["kind"] == "random"} >= full
    assert T.HALO_MAPS == [(1, 1), (8, 32), (9, 33), (3, 70)]
    for cin in (32, 64):
        for cout in (32, 64):
            for e in T.HALO_EPILOGUES:
                if e != "head" or cout == 32:
                    assert {c["a_relu"] for c in ha if (c["cin"], c["cout"], c["epi"]) == (cin, cout, e)} == {0, 1}
            assert any(not c["bias"] for c in ha if (c["cin"], c["cout"]) == (cin, cout))
    assert {c["kind"] for c in ha} == {"random", "positive"} and any(c["k_extra"] == 64 for c in ha)
    for c in ha:
        a = T.materialize(c)
        assert a["K"] == -(-9 * c["cin"] // 64) * 64 + c["k_extra"] and (a["epi"] == G.HEAD_OUT or a["ldo"] == c["cout"] + 8)
        if a["K"] > 9 * c["cin"]:
            assert (a["W"][:, 9 * c["cin"]:] == 512).all()  # the pad columns hold values the kernel must not read
    for c in T.all_cases():  # small shapes, B = 2 unless the case is about something else
        pixels = T.deform_m(c) if c["entry"] == "deform" else c["B"] * c["H"] * c["W"]
        assert pixels < 400 or (c["entry"] == "mbconv" and pixels <= 2 * 5 * 192) or (c["entry"] == "halo" and pixels <= 2 * 9 * 33), c["id"]  # (the issue's own maps at B = 2)


def test_numpy_packer_is_the_host_packer():
    lib = L.get_lib()
    rng = np.random.default_rng(3)
    rows = rng.standard_normal((64, 256)).astype(np.float16)
    packed = np.zeros(64 * 256, np.float16)
    L.vx_check(lib.vx_mbconv_pack_w3(rows.ctypes.data, packed.ctypes.data))
    np.testing.assert_array_equal(R.pack_w3(rows).view(np.uint16), packed.view(np.uint16))
    np.testing.assert_array_equal(R.unpack_w3(packed).view(np.uint16), rows.view(np.uint16))
    nt, s, lane, j = 1, 5, 37, 6  # the header, element by element
    assert packed[((nt * 16 + s) * 64 + lane) * 8 + j] == rows[nt * 32 + (lane & 31), (2 * s + (lane >> 5)) * 8 + j]
    assert lib.vx_mbconv_pack_w3(None, packed.ctypes.data) == 0 and b"null pointer" in lib.vx_last_error()


def _positions(a, c, k, pad):
    taps = k * k
    om = a["offset"] if c["entry"] == "deform" else a["om"]
    OH, OW = T.deform_extent(c) if c["entry"] == "deform" else (c["H"], c["W"])
    return D.deform_positions(om[:, :2 * taps].astype(np.float64).reshape(c["B"], OH, OW, 2 * taps), k, k, pad)


def test_planted_positions_are_what_they_claim():
    """the planted offsets do put samples at -1, H, H - 1/2, -1/2, W - 1/2, on an integer and far outside, for the first and the last tap of every
    case with planted data; and in the four cases of tests/test_gpu_graph_deform.py, whose check this is"""
    n = 0
    for c in T.group("deform") + T.group("cols"):
        a = T.materialize(c)
        if c["kind"] not in ("random", "positive"):
            assert not a["planted"]
            continue
        k = c["k"]
        pad = c["pad"] if c["entry"] == "deform" else k // 2
        H, W = c["H"], c["W"]
        py, px = _positions(a, c, k, pad)
        assert {p[0] for p in a["planted"]} == set(T.PLANTS) and {p[1] for p in a["planted"]} >= {0, k * k - 1} and len({p[1:] for p in a["planted"]}) == len(a["planted"])
        for what, tap, b, oy, ox in a["planted"]:
            y, x = py[tap, b, oy, ox], px[tap, b, oy, ox]
            ok = {"py=-1": y == -1, "py=H": y == H, "py=H-1/2": y == H - 0.5 and 0 <= x <= W - 1, "px=-1/2": x == -0.5 and 0 <= y <= H - 1,
                  "px=W-1/2": x == W - 0.5 and 0 <= y <= H - 1, "integer": y == int(y) and x == int(x) and 0 <= y < H and 0 <= x < W, "far": y < -20 and x < -1}[what]
            assert ok, (c["id"], what, tap, y, x)
            n += 1
    assert n > 1000
    import test_gpu_graph_deform as GD
    for case in GD.CASES:
        cin, cout, k, h, w, B = case
        off, pad, last = GD._operands(case)[2], k // 2, k * k - 1
        assert -pad + off[0, 0, 1, 0] == -1 and (h - 1 - pad + k - 1) + off[0, h - 1, 2, 2 * last] == h
        assert (h - 1 - pad + k - 1) + off[B - 1, h - 1, 3, 2 * last] == h - 0.5 and (w - 1 - pad + k - 1) + off[B - 1, 1, w - 1, 2 * last + 1] == w - 0.5
        assert float(np.float32(2 - pad) + np.float32(off[0, 2, 3, 0])).is_integer()
        assert np.array_equal(off, off.astype(np.float16).astype(np.float64))


def test_zero_offset_references_equal_the_plain_convolution():
    n = 0
    for c in T.group("deform"):
        if c["kind"] != "zero-offset":
            continue
        a = T.materialize(c)
        k = c["k"]
        want = R.deform(a)[0]
        plain = D.conv2d(a["x"].astype(np.float64), a["w"][:c["Cout"]].astype(np.float64).reshape(c["Cout"], k, k, c["Cin"]), None, c["pad"])
        np.testing.assert_allclose(want, plain.reshape(want.shape), rtol=0, atol=1e-12)
        n += 1
    assert n >= 2


def test_impulse_references_are_the_known_closed_forms():
    for c in T.group("deform") + T.group("cols"):
        if c["kind"] != "impulse":
            continue
        a = T.materialize(c)
        want = (R.deform(a) if c["entry"] == "deform" else R.cols(a))[0]
        OW = T.deform_extent(c)[1] if c["entry"] == "deform" else c["W"]
        row = ((c["B"] - 1) * (want.shape[0] // c["B"])) + T.IMPULSE_OUT[0] * OW + T.IMPULSE_OUT[1]
        col, value = a["hot"]
        if c["entry"] == "cols":
            value *= 2.0 * D.sigmoid((c["tap"] - 4) / 4.0)
        exp = np.zeros_like(want)
        exp[row, col] = value
        np.testing.assert_allclose(want, exp, rtol=0, atol=1e-12)
        assert value > 0.02
    weights = sorted({T.materialize(c)["hot"][1] for c in T.group("cols") if c["kind"] == "impulse"})
    assert len(weights) == 3 and weights[1] * 3 == weights[2] and weights[0] * 9 == weights[2]  # corners 1 and 2 differ by a factor of 9
    for c in T.group("mbconv"):
        if c["kind"] != "impulse":
            continue
        a = T.materialize(c)
        want = R.mbconv(a)[0]
        ky, kx = divmod(c["tap"], 3)
        exp = np.zeros_like(want)
        for i, (y, x) in enumerate(T.MB_IMPULSE_AT):  # out(y, x) = in(y + ky - 1, x + kx - 1)
            exp[-1, y + 1 - ky, x + 1 - kx, (7 * c["tap"] + 30 * i + 1) % 64] = R.gelu(R.gelu(3.0))
        np.testing.assert_allclose(want, exp, rtol=0, atol=1e-12)
    a = T.materialize(T.case("mbconv-w3-probe"))
    want = R.mbconv(a)[0]
    np.testing.assert_allclose(want, T.W3_PROBE_B2 + a["h"].astype(np.float64)[..., T.w3_probe_column(np.arange(64))], rtol=0, atol=1e-12)
    assert len(set(T.w3_probe_column(np.arange(64)).tolist())) == 64


# ---- 2. numpy emulations of the kernels' arithmetic, with the defects they can carry -------------------------------------------------------

def sample32(x, off, k, pad, factor, corrupt=None):
    """the samplers' A operand in their arithmetic: f32 positions, weights and blend, the product with the mask factor rounded to f16 once
    -> float64 [B, OH, OW, taps, C]"""
    B, H, W, C = x.shape
    OH, OW = off.shape[1:3]
    taps, one = k * k, F32(1)
    x32, off32 = x.astype(F32), off.astype(F32)
    oy, ox = np.meshgrid(np.arange(OH), np.arange(OW), indexing="ij")
    bi = np.arange(B)[:, None, None]
    out = np.zeros((B, OH, OW, taps, C))
    for t in range(taps):
        ky, kx = divmod(t, k)
        dy, dx = off32[..., 2 * t], off32[..., 2 * t + 1]
        if corrupt == "dy_dx_swapped":
            dy, dx = dx, dy
        py, px = (oy - pad + ky).astype(F32)[None] + dy, (ox - pad + kx).astype(F32)[None] + dx
        inside = (py > -1) & ((py <= H) if corrupt == "le_at_H" else (py < H)) & (px > -1) & (px < W)
        y0, x0 = np.floor(py).astype(np.int64), np.floor(px).astype(np.int64)
        ly, lx = py - y0.astype(F32), px - x0.astype(F32)
        wts = [(one - ly) * (one - lx), (one - ly) * lx, ly * (one - lx), ly * lx]
        if corrupt == "corners_1_2_swapped":
            wts[1], wts[2] = wts[2], wts[1]
        acc = np.zeros((B, OH, OW, C), F32)
        for (yy, xx), wgt in zip(((y0, x0), (y0, x0 + 1), (y0 + 1, x0), (y0 + 1, x0 + 1)), wts):
            ok = (yy >= 0) & (yy <= H - 1) & (xx >= 0) & (xx <= W - 1)
            v = x32[bi, np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1)]
            if corrupt != "corner_clamped":
                v = np.where(ok[..., None], v, F32(0))
            acc = acc + wgt[..., None] * v
        m = factor[..., (t + 1) % taps if corrupt == "mask_of_next_tap" else t]
        val = np.where(inside[..., None], acc * m[..., None], F32(0))
        assert val.dtype == F32
        out[:, :, :, t] = f16(val)
    return out


def _sigmoid32(v, scale):
    return F32(scale) / (F32(1) + np.exp(-v.astype(F32)))


def emulate_deform(a, corrupt=None):
    B, H, W, Cin, Cout, k, pad = (a[key] for key in ("B", "H", "W", "Cin", "Cout", "k", "pad"))
    taps, OH, OW = k * k, H + 2 * pad - k + 1, W + 2 * pad - k + 1
    M = B * OH * OW
    off = a["offset"][:, :2 * taps].reshape(B, OH, OW, 2 * taps)
    if a["mask_mode"] == 0:
        factor = np.ones((B, OH, OW, taps), F32)
    else:
        raw = (a["offset"][:, a["mask_col"]:a["mask_col"] + taps] if a["mask"] is None else a["mask"]).reshape(B, OH, OW, taps).astype(F32)
        factor = _sigmoid32(raw, a["mask_scale"]) if a["mask_mode"] == 2 else raw
    A = sample32(a["x"], off, k, k // 2 if corrupt == "pad_is_half_k" else pad, factor, corrupt).reshape(M, taps * Cin)
    if corrupt == "last_k_step_dropped":
        A[:, -T.deform_ck(Cin):] = 0
    acc = A.astype(F32) @ a["w"][:Cout].astype(F32).T
    if a["scale"] is not None:
        acc = acc * a["scale"]
    if a["bias"] is not None:
        acc = acc + a["bias"]
    if a["relu"]:
        acc = np.maximum(acc, F32(0))
    assert acc.dtype == F32
    return f16(acc)


def emulate_cols(a, corrupt=None):
    B, H, W, C, k = (a[key] for key in ("B", "H", "W", "C", "k"))
    taps = k * k
    off = a["om"][:, :2 * taps].reshape(B, H, W, 2 * taps)
    factor = _sigmoid32(a["om"][:, 2 * taps:3 * taps].reshape(B, H, W, taps), 2.0)
    return sample32(a["x"], off, k, k // 2, factor, corrupt).reshape(B * H * W, taps * C)


def gelu32(x):
    """vx_device.h's gelu_tanh in float32: x / (1 + exp2(x (c3 x^2 + c1)))"""
    c1 = F32(-2.0 * 0.79788456080286535588 * 1.44269504088896340736)
    c3 = c1 * F32(0.044715)
    with np.errstate(over="ignore"):
        return x * (F32(1) / (F32(1) + np.exp2(x * (x * x * c3 + c1))))


def emulate_mbconv(a, corrupt=None):
    h, w2 = a["h"].astype(F32), a["w2"].astype(F32)
    B, H, W, _ = h.shape
    hp = np.pad(h, ((0, 0), (1, 1), (1, 1), (0, 0)))
    acc = np.zeros_like(h)
    for t in range(9):
        ky, kx = divmod(t, 3)
        src = hp[:, ky:ky + H, kx:kx + W]
        if corrupt == "strip_seam_column" and kx == 0:  # the column left of a strip of 8 pixels holds the strip's first column
            first = np.arange(W) % 8 == 0
            src = np.where(first[None, None, :, None], hp[:, ky:ky + H, 1:1 + W], src)
        acc = acc + src * w2[t]
    g = f16(gelu32(acc + a["b2"])).astype(F32)
    w3 = a["w3_rows"].astype(F32)
    if corrupt == "w3_halves_swapped":  # the two 8-column halves of every k step (lane >> 5) change places
        w3 = w3.reshape(64, 16, 2, 8)[:, :, ::-1].reshape(64, 256)
    z = g @ w3.T + a["b3"] + a["x"].astype(F32)
    assert z.dtype == F32
    y = f16(gelu32(z))
    if corrupt == "remap_off_by_one":  # hardware block b computes segment order(b) + 1: segment 0 is never computed
        y.reshape(-1, 64)[:R.MB_PX] = 0
    return y


def emulate_halo(a, corrupt=None):
    B, H, W, cin = a["A"].shape
    N, epi = a["N"], a["epi"]
    x = a["A"].astype(F32)
    if a["a_relu"]:
        x = np.maximum(x, F32(0))
    xp = np.pad(x, ((0, 0), (1, 1), (1, 1), (0, 0)))
    w = a["W"][:, :9 * cin].astype(F32).reshape(N, 9, cin)
    acc = np.zeros((B, H, W, N), F32)
    for t in range(9):
        ky, kx = divmod(t, 3)
        src = xp[:, ky:ky + H, kx:kx + W]
        if corrupt == "top_halo_row" and ky == 0:  # a tile's halo row 0 holds its row 1: the first output row of every 8-row tile reads its own row
            src = np.where((np.arange(H) % 8 == 0)[None, :, None, None], xp[:, 1:1 + H, kx:kx + W], src)
        acc = acc + src @ w[:, t].T
    if a["bias"] is not None:
        acc = acc + a["bias"]
    v = acc.reshape(B * H * W, N)
    if epi == G.RELU or epi == G.HEAD_OUT or (epi == G.ADD and a.get("relu")):
        v = np.maximum(v, F32(0))
    v = f16(v)  # the staged tile
    if epi == G.HEAD_OUT:
        dot = np.zeros(v.shape[0], F32)
        for n in range(N):
            dot = dot + v[:, n].astype(F32) * a["lambda_"][n]
        return (np.maximum(dot + F32(a["head_bias"]), F32(0)) * F32(a["head_scale"])).astype(np.float64)
    if epi == G.ADD and a.get("res1") is not None:
        s = v.astype(F32) + a["res1"][:, :N].astype(F32)
        if a.get("res2") is not None:
            s = s + a["res2"][:, :N].astype(F32)
        v = f16(s)
    return v


EMULATE = {"deform": emulate_deform, "cols": emulate_cols, "mbconv": emulate_mbconv, "halo": emulate_halo}
_CACHE = {}


def _reference(c):
    """-> (args, want, allow), want and allow in the emulations' shape"""
    if c["id"] not in _CACHE:
        a = T.materialize(c)
        if c["entry"] == "halo":
            want, allow, _ = G.evaluate(a)
            want, allow = (v["out"] if a["epi"] == G.HEAD_OUT else v["out"][:, :a["N"]] for v in (want, allow))
        else:
            want, allow = {"deform": R.deform, "cols": R.cols, "mbconv": R.mbconv}[c["entry"]](a)[:2]
        _CACHE[c["id"]] = (a, want, allow)
    return _CACHE[c["id"]]


def _outside(c, corrupt=None):
    """elements of the emulation that buffer_check.violations rejects, and the largest error / allowance"""
    a, want, allow = _reference(c)
    v = violations(EMULATE[c["entry"]](a, corrupt), (want, allow, np.ones(want.shape, bool)))  # the GPU test's comparison (a NaN is outside)
    return v["nonfinite"] + v["outside"], v["ratio"]


def test_emulated_arithmetic_is_inside_the_allowance_for_every_case():
    worst = defaultdict(float)
    for c in T.all_cases():
        n_bad, ratio = _outside(c)
        assert n_bad == 0, (c["id"], n_bad, ratio)
        worst[(c["entry"], c["kind"])] = max(worst[(c["entry"], c["kind"])], ratio)
    print("\nlargest emulated error / allowance per entry point and data kind:")
    for k, v in sorted(worst.items()):
        print(f"  {k[0]:8s} {k[1]:12s} {v:.3f}")
    # the allowance is no blanket: every output is rounded to f16 on the way out, and where nothing exp-based loosens it the emulation comes
    # within a factor of a few of it
    assert worst[("deform", "positive")] > 0.25 and worst[("deform", "random")] > 0.25 and worst[("halo", "positive")] > 0.25 and worst[("mbconv", "positive")] > 0.1


WRONG_KERNELS = [
    ("dy_dx_swapped", ["deform-cin16", "deform-cin48-pos", "deform-impulse-tap0-corner1", "deform-impulse-tap8-corner2", "cols-c8-k3-exact-pos", "cols-impulse-tap3-corner2"]),
    ("corners_1_2_swapped", ["deform-cin16-pos", "deform-impulse-tap4-corner1", "deform-impulse-tap0-corner2", "cols-impulse-tap8-corner1", "cols-c24-k3-pad8-pos"]),
    ("corner_clamped", ["deform-k3p2-pos", "deform-k7p3-4x6-pos", "deform-cin48-pos", "cols-c8-k7-exact-pos"]),
    ("mask_of_next_tap", ["deform-cin96-pos", "deform-impulse-tap3-corner0", "deform-mask1-separate", "cols-c8-k3-exact-pos", "cols-impulse-tap2-corner3"]),
    ("last_k_step_dropped", ["deform-cin48-pos", "deform-cin96-pos", "deform-cin80-pos", "deform-cin160-pos", "deform-cin128-pos", "deform-k2p0-pos", "deform-zero-offset-k4p1-cin48"]),
    ("pad_is_half_k", ["deform-k3p0-pos", "deform-k3p2-pos", "deform-k2p0-pos", "deform-k4p1-pos", "deform-k7p0-pos", "deform-zero-offset-k4p1-cin48"]),
    ("strip_seam_column", ["mbconv-impulse-tap0", "mbconv-impulse-tap3", "mbconv-impulse-tap6", "mbconv-1x1x64-pos", "mbconv-2x5x192-pos"]),
    ("w3_halves_swapped", ["mbconv-w3-probe", "mbconv-1x2x64-pos", "mbconv-3x5x64"]),
    ("remap_off_by_one", ["mbconv-1x1x64-pos", "mbconv-2x3x64-pos", "mbconv-1x8x128", "mbconv-2x5x192-pos"]),
    ("top_halo_row", ["halo-32-32-1x1-f16-arelu", "halo-64-64-9x33-f16-pos", "halo-32-64-3x70-add-res12-arelu", "halo-64-32-8x32-head", "halo-64-32-9x33-head-pos"]),
]
# `<=` instead of `<` at py = H changes nothing in these kernels: at py = H the cell is (H, H + 1), both rows lie outside the map, and a corner
# outside the map counts as zero whatever the inside test says (likewise `>=` at py = -1: the row inside has weight ly = 0). No case can
# separate it; the test below pins that the model gives the correct emulation's bits, so that nobody takes the planted py = H for a test of it.
EQUIVALENT_KERNELS = [("le_at_H", ["deform-cin16", "deform-k7p3-4x6-pos", "deform-k3p2", "cols-c8-k3-exact"])]


def test_the_wrong_kernel_table_lists_every_model():
    assert [w for w, _ in WRONG_KERNELS] + [w for w, _ in EQUIVALENT_KERNELS] == [
        "dy_dx_swapped", "corners_1_2_swapped", "corner_clamped", "mask_of_next_tap", "last_k_step_dropped", "pad_is_half_k", "strip_seam_column",
        "w3_halves_swapped", "remap_off_by_one", "top_halo_row", "le_at_H"]


@pytest.mark.parametrize("what,ids", WRONG_KERNELS, ids=[w for w, _ in WRONG_KERNELS])
def test_modelled_wrong_kernels_are_outside_the_allowance(what, ids):
    for cid in ids:
        c = T.case(cid)
        assert _outside(c)[0] == 0, (what, cid)
        assert _outside(c, what)[0] > 0, (what, cid)


@pytest.mark.parametrize("what,ids", EQUIVALENT_KERNELS, ids=[w for w, _ in EQUIVALENT_KERNELS])
def test_inclusive_bound_at_py_equal_h_cannot_show(what, ids):
    for cid in ids:
        c = T.case(cid)
        a = _reference(c)[0]
        assert any(p[0] == "py=H" for p in a["planted"])
        np.testing.assert_array_equal(EMULATE[c["entry"]](a, what), EMULATE[c["entry"]](a))


# ---- 3. the refusals ----------------------------------------------------------------------------------------------------------------------------

def test_refusal_tables_return_before_any_launch():
    """host code: every refusal is decided before the first HIP call, so the tables run without a device (the operands are one host buffer)"""
    if L.get_lib().vx_device_count() > 0:
        return  # with a device the GPU suite runs the tables, on device memory (a refusal that regressed would launch on these host operands)
    scratch = np.zeros(T.REFUSAL_SCRATCH_BYTES, np.uint8)
    seen = []
    assert T.run_refusals(L.get_lib(), scratch.ctypes.data, seen) == len(T.DEFORM_REFUSALS) + len(T.MBCONV_REFUSALS) + len(T.HALO_REFUSALS) + len(T.COLS_REFUSALS) > 70
    assert not scratch.any()
    # every VX_REQUIRE of the deformable conv's launcher has produced its message
    src = (Path(__file__).resolve().parents[1] / "vision.cpp_amd" / "csrc" / "kernels_deform.hip").read_text()
    formats = re.findall(r'VX_REQUIRE\(.*?"(vx_deform_conv_f16: [^"]*)"', src, re.S)
    assert len(formats) == src.count("VX_REQUIRE(") == 10
    for fmt in formats:
        pattern = re.sub(r"%l?d", r"-?\\d+", re.escape(fmt).replace("%%", "%"))
        assert any(re.fullmatch(pattern, m) for m in seen), fmt
    kinds = {m for _, m in T.DEFORM_REFUSALS}
    assert {"null operand", "input too large", "must be 16-byte aligned", "offset rows of 17 elements hold fewer than 2 x 9 taps"} <= kinds
    assert {m for _, m in T.HALO_REFUSALS} >= {"conv_pix", "post_gelu", "window-order", "k_splits", "ld_res1", "a_group"}
    assert any("kernel 2" in m for _, m in T.COLS_REFUSALS) and any("offset row stride 26" in m for _, m in T.COLS_REFUSALS)

"""No device: the references of tests/pixel_ref.py agree with the CPU oracle, the tables of tests/pixel_cases.py reach every dispatch class of
every launcher (the launchers' `if` chains are checked against the source text), a float32 numpy emulation of each kernel's arithmetic lies
inside the allowance for EVERY case, emulations with one seeded mistake each are rejected by the comparison the GPU test uses
(buffer_check.violations, and its u8 twin for the byte outputs), and the refusal tables return before any launch. No element and no case is
exempt anywhere in this file."""
import re
from collections import defaultdict
from pathlib import Path

import numpy as np
import pytest

import pixel_cases as T
import pixel_ref as R
from buffer_check import rejected, violations
from oracle import oracle
from visioncpp_amd import _lib as L

F32 = np.float32
CSRC = Path(__file__).resolve().parents[1] / "vision.cpp_amd" / "csrc"


def _args():
    """every case materialised once (the largest holds 8.4 M f16 values)"""
    if not _args.cache:
        _args.cache = {c["id"]: T.materialize(c) for c in T.all_cases()}
    return _args.cache


_args.cache = {}


def args_of(c):
    return _args()[c["id"]]


# ---- 1. the references against the oracle -----------------------------------------------------------------------------------------------------

def _oracle_norm(img, mean, inv):
    return oracle.image_u8_to_f32(img, oracle.RGB_U8, oracle.RGB_F32, tuple(-np.asarray(mean, np.float64)) + (0,), tuple(np.asarray(inv, np.float64)) + (1,))


@pytest.mark.parametrize("cid", ["patches-ps14-kp592-2x3-b3-random-imagenet", "patches-ps8-kp200-3x2-b1-ramp-identity", "patches-ps3-kp32-6x6-b1-ramp-imagenet",
                                 "pre32-b2-3x5-imagenet", "pre32-b1-600x600-identity"])
def test_normalisation_matches_image_u8_to_f32(cid):
    """the oracle evaluates the same three f32 operations: it lies inside the f32 allowance; the patch rows are its pixels in (ky, kx, c) order"""
    c = T.case(cid)
    a = args_of(c)
    B, H, W = a["B"], a["H"], a["W"]
    got = np.stack([_oracle_norm(a["rgb"][b].reshape(H, W, 3), a["mean"], a["inv"]) for b in range(B)]).astype(np.float64)
    p, e = R.norm_div(a["rgb"].reshape(B, H, W, 3), a["mean"], a["inv"])
    assert (np.abs(got - p) <= e).all()
    if c["entry"] == "patches":
        ps, kreal = a["ps"], a["ps"] ** 2 * 3
        want = R.patches(a)[0]
        rows = got.reshape(B, H // ps, ps, W // ps, ps, 3).transpose(0, 1, 3, 2, 4, 5).reshape(-1, kreal)
        assert (np.abs(rows - want[:, :kreal]) <= e.max()).all() and not want[:, kreal:].any()


def test_value_and_residue_pixels_match_the_oracle():
    for cid in ("tvpre-n257-ramp", "tvpre-n255-random"):
        a = args_of(T.case(cid))
        got = _oracle_norm(a["rgb"].reshape(1, -1, 3), (0.485, 0.456, 0.406), (1 / 0.229, 1 / 0.224, 1 / 0.225)).reshape(-1, 3)
        p, e = R.norm_div(a["rgb"], R.IMAGENET_MEAN, R.IMAGENET_INV)
        assert (np.abs(got - p) <= e + R.U32 * np.abs(p)).all()  # (the oracle is handed 1 / std rounded from float64: one more unit)
        want, allow = R.tvpre(a)
        assert (np.abs(R.f16(want[:, :3]) + want[:, 3:6] - p) <= 1e-15).all() and (np.abs(want[:, 3:6]) <= R.U16 * np.abs(p) + R.TINY16).all() and not want[:, 6:].any()


@pytest.mark.parametrize("cid", ["bfhalf-b2-4x6-random", "bfhalf-b1-6x10-random", "bfhalf-b1-64x96-random", "bfhalf-b2-2x8-ramp"])
def test_half_size_resize_matches_interpolate_nhwc(cid):
    a = args_of(T.case(cid))
    B, H, W = a["B"], a["H"], a["W"]
    p, e = R.norm_mul(a["rgb"].reshape(B, H, W, 3))
    v, e32 = R.bilinear_half(p, e)
    got = oracle.interpolate_nhwc(p.astype(F32), (H // 2, W // 2), "bilinear", True).astype(np.float64)
    assert (np.abs(got - v) <= e32 + R.U32 * np.abs(p).max()).all()  # (the oracle starts from p rounded to f32)


@pytest.mark.parametrize("cid", ["bfpatches-g2x4-5x7-b2", "bfpatches-g3x3-8x12-b1", "bfpatches-g8x8-5x7-b1"])
def test_image_patches_match_image_to_patches(cid):
    a = args_of(T.case(cid))
    B, h, w, gh, gw = (a[k] for k in ("B", "h", "w", "gh", "gw"))
    p, _ = R.norm_mul(a["rgb"].reshape(B, gh * h, gw * w, 3))
    got = np.stack([oracle.image_to_patches(p[b].astype(F32), w, h) for b in range(B)]).reshape(B * h * w, -1)
    assert np.array_equal(got, R.bfpatches(a)[0].astype(F32))


def test_minmax_reference_matches_image_normalize():
    for cid in ("minmax-b3-n1027-mixed", "minmax-b4-n1028-negative-kinds", "minmax-b3-n1027-const-kinds", "minmax-b4-n1028-above-kinds", "minmax-b3-n1027-below-kinds", "minmax-b17-n255-mixed"):
        a = args_of(T.case(cid))
        want, allow, at_min = R.minmax(a)
        for b in range(a["B"]):
            got = oracle.image_normalize(a["d"][b].reshape(1, -1)).reshape(-1).astype(np.float64)
            assert (np.abs(got - want[b]) <= np.maximum(allow[b], R.U32 * 4 * np.abs(want[b]))).all(), (cid, b)  # (the oracle may round the minimum's own terms)
        assert at_min.any(axis=1).all() and not want[at_min].any()


def test_f32_to_u8_reference_matches_image_f32_to_u8():
    v = T.u8_values()
    finite = v[~np.isnan(v)]
    got = oracle.image_f32_to_u8(finite.reshape(1, -1, 1), oracle.ALPHA_F32, oracle.ALPHA_U8).reshape(-1)
    np.testing.assert_array_equal(got, R.f32_to_u8(finite))
    want = R.f32_to_u8(v)
    assert want[np.isnan(v)].tolist() == [0] and set(want.tolist()) == set(range(256))
    k = np.arange(256)
    centre = want[:1280].reshape(256, 5)
    assert ((centre == k[:, None]) | (centre == k[:, None] - 1)).all() and (centre != k[:, None]).any()  # the neighbourhoods straddle their code boundaries


@pytest.mark.parametrize("cid", ["sam-up-f16-f32", "sam-down-f32-f32", "sam-identity-f16-f32", "sam-wide-f32-f32", "sam-tall-f16-f32"])
def test_sam_reference_matches_interpolate_nhwc(cid):
    """half-pixel centres, the source clamped at 0: interpolate(align_corners = false)"""
    a = args_of(T.case(cid))
    src = R.sam_source(a)
    v, e = R.sam_values(a)
    got = oracle.interpolate_nhwc(src.astype(F32)[None, :, :, None], (a["dh"], a["dw"]), "bilinear", False)[0, :, :, 0].astype(np.float64)
    # the oracle may state its coordinate otherwise: its f32 coordinate differs by a few units of the largest coordinate, times the steepest slope
    slack = 8 * R.U32 * max(a["sw"], a["sh"]) * 2 * np.abs(src).max()
    assert (np.abs(got - v) <= e + slack).all()
    if a["sw"] == a["dw"] and a["sh"] == a["dh"]:
        assert np.array_equal(v, src)


def test_no_u8_pixel_of_the_sam_table_is_undecided():
    n = 0
    for c in T.group("sam"):
        if c["out_u8"]:
            a = args_of(c)
            assert R.sam_undecided(a) == 0, c["id"]
            v, _ = R.sam_values(a)
            assert (v > 0).any() and (v <= 0).any(), c["id"]
            n += 1
    assert n == 14


# ---- 2. the tables ---------------------------------------------------------------------------------------------------------------------------------

def test_tables_span_what_the_issue_names():
    g = T.group
    pa = g("patches")
    assert {(c["ps"], c["Kp"]) for c in pa} == {(14, 592), (16, 768), (8, 192), (8, 200), (3, 32), (1, 8)}
    for ps, Kp in T.PATCH_SIZES:
        mine = [c for c in pa if (c["ps"], c["Kp"]) == (ps, Kp)]
        assert {(c["H"] // ps, c["W"] // ps, c["B"], c["kind"], c["norm"]) for c in mine} >= {(ph, pw, B, k, nm) for ph, pw in ((1, 1), (2, 3), (3, 2)) for B in (1, 3) for k in ("ramp", "random") for nm in T.NORMS}
        assert any(c["kind"] == "ramp" and all(len(set(args_of(c)["rgb"][b, :, ch].tolist())) == 256 for b in range(c["B"]) for ch in range(3)) for c in mine), ps
    assert 768 == 16 * 16 * 3 and 192 == 8 * 8 * 3 and 592 > 14 * 14 * 3 and 32 > 27 and 8 > 3  # no padding at 16 and at (8, 192), padding elsewhere
    assert {(c["B"], c["H"], c["W"]) for c in g("pre32")} == {(1, 1, 1), (2, 3, 5), (1, 600, 600)} and {c["norm"] for c in g("pre32")} == set(T.NORMS)
    assert {(c["B"], c["T"], c["C"]) for c in g("cls")} == {(B, Tt, C) for B in (1, 3) for Tt in (1, 2, 5) for C in (1, 96, 128, 130, 384, 1024)}
    ho = g("head_out")
    assert {(c["C"], c["n"], c["max_depth"]) for c in ho} >= {(C, n, md) for C in (8, 16, 32, 64) for n in (1, 255, 257) for md in (1.0, 80.0, 0.5)}
    assert {c["n"] for c in ho if c["n"] > 257} == {4096 * 256 + 3} and {c["C"] for c in ho if c["n"] > 257} == {8}
    assert {c["bias"] > 0 for c in ho} == {True, False} and {c["C"] for c in ho if c["kind"] == "negative"} == {8, 16, 32, 64}
    mm = g("minmax")
    assert {(c["B"], c["n"]) for c in mm if c["kind"] == "mixed"} >= {(B, n) for B in (1, 3, 4, 5, 16, 17) for n in (1, 3, 4, 5, 255, 1027, 70001)}
    for shape in T.MINMAX_KIND_SHAPES:
        assert {c["kind"] for c in mm if (c["B"], c["n"]) == shape} == set(T.MINMAX_KINDS)
    assert {c["n"] for c in g("u8")} == {1, 257, 4096 * 256 + 3}
    assert {c["n"] for c in g("tvpre")} == {1, 255, 256, 257}
    assert {(c["H"], c["W"], c["B"]) for c in g("bfhalf")} == {(H, W, B) for H, W in ((2, 2), (2, 8), (4, 6), (6, 10), (64, 96)) for B in (1, 2)}
    assert {H // 2 % 2 for H, _ in T.BFHALF_HW} == {0, 1} == {W // 2 % 2 for _, W in T.BFHALF_HW}
    bp = g("bfpatches")
    assert {(c["gw"], c["gh"], c["h"], c["w"], c["B"]) for c in bp} == {(gw, gh, h, w, B) for gw, gh in ((1, 1), (2, 2), (3, 3), (2, 4), (4, 4), (8, 8)) for h, w in ((5, 7), (8, 12)) for B in (1, 2)}
    assert sorted({3 * c["gw"] * c["gh"] for c in bp}) == [3, 12, 24, 27, 48, 192]
    sm = g("sam")
    assert {(c["resize"], c["src_f16"], c["out_u8"]) for c in sm} == {(r, s, o) for r in T.SAM_RESIZES for s in (0, 1) for o in (0, 1)}
    rs = T.SAM_RESIZES
    assert rs["up"] == (16, 16, 64, 64) and rs["down"] == (64, 48, 40, 24) and rs["identity"][:2] == rs["identity"][2:] and rs["dw1"][2] == 1 and rs["sw1"][0] == 1
    assert rs["wide"][2] < rs["wide"][3] and rs["tall"][2] > rs["tall"][3]
    for c in sm:
        a = args_of(c)
        assert (a["step"], a["offset"], a["sstride"] == a["sw"]) == ((8, 2, True) if c["src_f16"] else (1, 0, False))


def test_every_dispatch_class_is_hit_and_the_restated_chains_are_the_sources():
    misc, bf, tv, common = ((CSRC / n).read_text() for n in ("kernels_misc.hip", "kernels_birefnet.hip", "kernels_tinyvit.hip", "vx_common.h"))
    # the restatements against the text
    assert re.search(r"if \(ps == 14\)\s+hipLaunchKernelGGL\(preprocess_patches_kernel<14>.*?else\s+hipLaunchKernelGGL\(preprocess_patches_kernel<0>", misc, re.S)
    assert "const int ps = PS ? PS : ps_rt;" in misc
    for C in T.HEAD_OUT_WIDTHS:
        assert f"head_out_kernel<{C}>" in misc
    assert "VX_REQUIRE(C == 8 || C == 16 || C == 32 || C == 64," in misc and sorted(set(re.findall(r"head_out_kernel<(\d+)>", misc))) == ["16", "32", "64", "8"]
    assert misc.count("grid_stride_blocks(n, 256 * 16)") == 2 and "grid_stride_blocks(n_pixels, 256 * 16)" in misc and 256 * 16 == R.GRID_CAP and "int per_block = 256" in common
    assert "return (int)(b < 1 ? 1 : (b > cap ? cap : b));" in common
    assert "int gx = grid_stride_blocks(n, 64);" in misc and "const int gmm = B >= 16 ? 16 : (B >= 4 ? 32 : 64);" in misc and "dim3(gmm < gx ? gmm : gx, B)" in misc and T.MINMAX_CAP == 64
    assert "(reinterpret_cast<uintptr_t>(d) & 15) == 0) ? n / 4 : 0" in misc and "delta = delta < 1e-5f ? 1.0f : delta;" in misc
    assert "if (CP % 8 == 0) *reinterpret_cast<f16x8*>(out + pix * CP + ch0) = o;" in bf and "for (int j = 0; j < 8 && ch0 + j < CP; ++j) out[pix * CP + ch0 + j] = o[j];" in bf
    assert "tv_sam_interp_kernel<f16>" in tv and "tv_sam_interp_kernel<float>" in tv and "if (out_u8) reinterpret_cast<uint8_t*>(dst)[i] = v > 0.0f ? 255 : 0;" in tv
    assert "dim3(B), dim3(128)" in misc  # write_cls_kernel: one block of 128 threads per image
    # the tables against the restatements
    assert {T.patches_instance(c["ps"]) for c in T.group("patches")} == {"ps14", "runtime"}
    assert {-(-(c["H"] // c["ps"]) * (c["W"] // c["ps"]) * (c["Kp"] // 8) // 256) > 1 for c in T.group("patches")} == {True, False}  # one block per image, and more
    assert {c["C"] for c in T.group("head_out")} == set(T.HEAD_OUT_WIDTHS)
    for name, count in (("pre32", lambda c: c["B"] * c["H"] * c["W"] * 3), ("head_out", lambda c: c["n"]), ("u8", lambda c: c["n"])):
        assert {T.loops(count(c)) for c in T.group(name)} == {True, False}, name
        assert {T.stride_blocks(count(c)) < R.GRID_CAP for c in T.group(name)} == {True, False}, name  # grids below the cap and at it
    assert T.stride_blocks(0) == 1 and T.stride_blocks(256) == 1 and T.stride_blocks(257) == 2 and T.stride_blocks(10 ** 9) == 4096 and not T.loops(4096 * 256) and T.loops(4096 * 256 + 1)
    mm = T.group("minmax")
    assert {T.minmax_class(c["B"]) for c in mm} == {16, 32, 64}
    assert {T.minmax_grids(c["B"], c["n"]) for c in mm} >= {(1, 1), (5, 5), (16, 64), (32, 64), (64, 64)}  # the cap of the image and the class's own, each class
    assert {T.loops(c["n"], T.MINMAX_CAP) for c in mm} == {True, False} and {c["n"] // 4 > T.minmax_grids(c["B"], c["n"])[0] * 256 for c in mm} == {True, False}  # both kernels stride
    aligned = {(T.image_aligned(b, c["n"]), c["n"] % 4 > 0, c["n"] >= 4) for c in mm for b in range(c["B"])}
    assert aligned >= {(True, False, True), (True, True, True), (True, True, False), (False, True, True), (False, True, False)}  # body only | body + tail | tail only | scalar
    for kind in T.MINMAX_KINDS:  # every data kind on the 16-byte path and on the scalar path
        assert {T.image_aligned(b, c["n"]) for c in mm if c["kind"] == kind for b in range(c["B"])} == {True, False}, kind
    assert {T.bf_patches_path(3 * c["gw"] * c["gh"]) for c in T.group("bfpatches")} == {"vector", "scalar-partial", "scalar-full+partial"}
    assert {-(-c["B"] * c["h"] * c["w"] * -(-3 * c["gw"] * c["gh"] // 8) // 256) > 1 for c in T.group("bfpatches")} == {True, False}
    assert {(c["src_f16"], c["out_u8"]) for c in T.group("sam")} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert {c["C"] > 128 for c in T.group("cls")} == {True, False} and any(c["C"] % 128 for c in T.group("cls") if c["C"] > 128)
    assert {-(-c["n"] // 256) for c in T.group("tvpre")} == {1, 2} and {-(-c["B"] * (c["H"] // 2) * (c["W"] // 2) // 256) > 1 for c in T.group("bfhalf")} == {True, False}


def test_data_kinds_are_what_they_claim():
    last_of_last = defaultdict(set)
    where = defaultdict(set)
    for c in T.group("minmax"):
        d = args_of(c)["d"]
        B, n, kind = c["B"], c["n"], c["kind"]
        assert np.isfinite(d).all() and d.dtype == F32 and d.shape == (B, n)
        if kind == "negative":
            assert (d < 0).all()
        elif kind == "mixed" and n > 1:
            assert (d.min(axis=1) < 0).all() and (d.max(axis=1) > 0).all()
        elif kind == "zeros":
            assert (d >= 0).all() and (d.min(axis=1) == 0).all() and np.signbit(d[d == 0]).any() and not np.signbit(d[d == 0]).all()
        elif kind == "subnormal":
            assert (np.abs(d) < np.finfo(F32).tiny).all() and (d != 0).all() and (d < 0).any() and (d > 0).any()
        elif kind == "huge":
            assert np.abs(d).max() > 1e30 and np.isfinite(d.max(axis=1) - d.min(axis=1)).all()
        elif kind in ("const0", "const"):
            assert (np.ptp(d, axis=1) == 0).all() and bool(d.any()) == (kind == "const")
        elif kind in ("below", "above"):
            delta = d.max(axis=1) - d.min(axis=1)
            assert delta.dtype == F32 and ((delta < F32(1e-5)) == (kind == "below")).all() and (delta >= np.nextafter(F32(1e-5), F32(0))).all()
        if kind in ("mixed", "negative", "huge"):
            for b in range(B):
                pmin, pmax = T.planted(c, b)
                assert d[b].argmin() == pmin and (n == 1 or d[b].argmax() == pmax) and (n == 1 or len(set(d[b].tolist())) > 1)
                names = {0: "first", n - 1: "tail", 4 * (n // 4) - 1: "body-end"}
                for p in (pmin, pmax):
                    where[names.get(p, "middle")].add(kind)
                if b == B - 1 and n - 1 in (pmin, pmax):
                    last_of_last[kind].add((B, n))
            if B > 1 and n > 1:
                assert len(set(d.min(axis=1).tolist())) == B  # every image has extremes of its own: a per-batch min/max is another function
    assert all(where[k] >= {"mixed"} for k in ("first", "tail", "body-end", "middle")) and last_of_last["mixed"] and last_of_last["huge"]
    for c in T.group("head_out"):
        a = args_of(c)
        want, _, decided = R.head_out(a)
        if c["kind"] == "negative":
            assert decided.all() and not want.any()
        elif c["n"] > 1:
            assert decided.any() and (want > 0).any()
    for c in T.group("sam"):
        a = args_of(c)
        assert np.isnan(a["src"]).sum() == a["src"].size - a["sw"] * a["sh"] and np.isfinite(R.sam_source(a)).all()  # what the call must not read is NaN


def test_the_canary_is_no_value_a_call_writes_and_the_guard_is_a_block():
    n = 0
    for c in T.all_cases():
        a = args_of(c)
        guard = T.guard_of(c, a)
        want, allow, written = R.evaluate(c["entry"], a, guard)
        assert np.isfinite(want).all() and np.isfinite(allow).all() and (allow >= 0).all()
        if R.out_dtype(c["entry"], a) == np.uint8:
            assert not allow.any() and (want[~written] == R.CANARY_U8).all()
        else:
            assert (np.abs(want - R.CANARY) > allow + 1000)[written].all(), c["id"]
        assert not written[-guard:].any() and (want[-guard:] == (R.CANARY_U8 if R.out_dtype(c["entry"], a) == np.uint8 else R.CANARY)).all() and not allow[~written].any()
        assert guard >= R.min_guard(c["entry"], a) >= 128
        if c["entry"] == "cls":
            assert written.sum() == c["B"] * c["C"] and np.array_equal(want[:-guard][~written[:-guard]], a["x"].reshape(-1).astype(np.float64)[~written[:-guard]])
        else:
            assert written[:-guard].all()
        z = R.zero_bit_elements(c["entry"], a, want.size)
        assert not want[z].any() and written[z].all() and not allow[z].any()
        if c["entry"] != "head_out" or c["n"] > 1:  # (a single pixel's pre-activation has either sign)
            assert z.any() == (c["entry"] in ("tvpre", "bfhalf", "minmax", "head_out") or (c["entry"] == "patches" and c["Kp"] > 3 * c["ps"] ** 2)), c["id"]
        n += 1
    assert n == len(T.all_cases()) > 350


# ---- 3. float32 emulations of the kernels, with the defects they can carry ---------------------------------------------------------------------

def _lut(mean, inv):
    u = np.arange(256, dtype=F32)[None, :]
    t = (u / F32(255) - mean.astype(F32)[:, None]) * inv.astype(F32)[:, None]
    assert t.dtype == F32
    return t  # [3, 256]


def _norm_px_f32(u):
    """kernels_birefnet.hip's norm_px without contraction"""
    t = (u.astype(F32) * (F32(1) / F32(255)) - R.IMAGENET_MEAN) * R.IMAGENET_INV
    assert t.dtype == F32
    return t


def _residue_f32(v):
    """vx_device.h's residue_pixel on v f32 [n, 3] -> f16 [n, 8]"""
    out = np.zeros((v.shape[0], 8), np.float16)
    hi = v.astype(np.float16)
    out[:, :3], out[:, 3:6] = hi, (v - hi.astype(F32)).astype(np.float16)
    return out


def _f2ord(f, negative_branch=True):
    u = f.view(np.uint32)
    neg = (u & np.uint32(0x80000000)) != 0
    return np.where(neg & negative_branch, ~u, u | np.uint32(0x80000000))


def _ord2f(u):
    u = np.asarray(u, np.uint32)
    return np.where((u & np.uint32(0x80000000)) != 0, u & np.uint32(0x7fffffff), ~u).astype(np.uint32).view(F32)


def _first_pass(values, defect):
    """`first_pass_only`: a grid-stride loop that stops after its first pass leaves the rest at the canary"""
    return R.GRID_CAP * R.BLOCK if defect == "first_pass_only" else values


def emulate(c, a, guard, defect=None):
    """-> the whole output buffer as evaluate() lays it out, in the output type"""
    e = c["entry"]
    size = R.evaluate(e, a, guard)[0].size
    buf = R.initial_buffer(e, a, size)
    body = buf[:size - guard]
    with np.errstate(over="ignore", invalid="ignore"):
        if e in ("patches", "pre32"):
            B, H, W = a["B"], a["H"], a["W"]
            lut = _lut(a["mean"], a["inv"])
            px = lut[np.arange(3)[None, None, None, :], a["rgb"].reshape(B, H, W, 3)]
            if e == "pre32":
                n = _first_pass(px.size, defect)
                body[:n] = px.reshape(-1)[:n]
            else:
                ps, Kp, kreal = a["ps"], a["Kp"], a["ps"] ** 2 * 3
                order = (0, 1, 3, 2, 5, 4) if defect == "channel_order_ky_c_kx" else (0, 1, 3, 2, 4, 5)
                rows = body.reshape(-1, Kp)
                rows[:, :kreal] = px.astype(np.float16).reshape(B, H // ps, ps, W // ps, ps, 3).transpose(order).reshape(-1, kreal)
                if defect != "pad_columns_unwritten":
                    rows[:, kreal:] = 0
        elif e == "cls":
            rows = body.reshape(a["B"] * a["T"], a["C"])
            rows[slice(None) if defect == "cls_on_every_row" else slice(None, None, a["T"])] = a["cls"] + a["pos"][:a["C"]]
        elif e == "head_out":
            x, w = a["x"].astype(F32), a["w"]
            acc = np.zeros(a["n"], F32)
            for ch in range(a["C"]):
                acc = acc + x[:, ch] * w[ch]
            v = np.maximum(acc + F32(a["bias"]), F32(0)) * F32(a["max_depth"])
            assert v.dtype == F32
            n = _first_pass(a["n"], defect)
            body[:n] = v[:n]
        elif e == "minmax":
            d = a["d"]
            seen = d
            if defect == "tail_missing_in_the_reduction":  # the n % 4 elements behind the 16-byte body of an aligned image
                seen = d.copy()
                for b in range(a["B"]):
                    if T.image_aligned(b, a["n"]) and a["n"] >= 4 and a["n"] % 4:
                        seen[b, 4 * (a["n"] // 4):] = seen[b, 0]
            o = _f2ord(seen, defect != "encoding_without_negative_branch")
            mn, mx = _ord2f(o.min(axis=1)), _ord2f(o.max(axis=1))
            if defect == "min_max_per_batch":
                mn, mx = np.full_like(mn, mn.min()), np.full_like(mx, mx.max())
            delta = mx - mn
            delta = np.where(delta < F32(1e-5), F32(1), delta)
            scale = F32(1) / delta
            offset = -mn * scale
            if defect == "normalisation_contracted":
                v = (d.astype(np.float64) * scale[:, None] + offset[:, None]).astype(F32)
            else:
                v = d * scale[:, None] + offset[:, None]
            assert v.dtype == F32
            body[:] = v.reshape(-1)
        elif e == "u8":
            v = np.fmin(np.fmax(a["src"], F32(0)), F32(1)) * F32(255)
            v = np.rint(v) if defect == "rounding_not_truncation" else v
            n = _first_pass(a["n"], defect)
            body[:n] = v.astype(np.uint8)[:n]
        elif e == "tvpre":
            lut = _lut(R.IMAGENET_MEAN, R.IMAGENET_INV)
            body[:] = _residue_f32(lut[np.arange(3)[None, :], a["rgb"]]).reshape(-1)
        elif e == "bfhalf":
            B, H, W = a["B"], a["H"], a["W"]
            OH, OW = H // 2, W // 2
            p = _norm_px_f32(a["rgb"].reshape(B, H, W, 3))

            def axis(n, on):
                f = np.arange(on).astype(F32) * (F32(n - 1) / F32(on - 1)) if on > 1 else np.zeros(1, F32)
                i0 = np.minimum(f.astype(np.int64), n - 1)
                return i0, np.minimum(i0 + 1, n - 1), f - i0.astype(F32)
            y0, y1, ty = axis(H, OH)
            x0, x1, tx = axis(W, OW)
            ty, tx = ty[None, :, None, None], tx[None, None, :, None]
            A, Bq, Cq, D = p[:, y0][:, :, x0], p[:, y0][:, :, x1], p[:, y1][:, :, x0], p[:, y1][:, :, x1]
            top, bot = A + (Bq - A) * tx, Cq + (D - Cq) * tx
            v = top + (bot - top) * ty
            assert v.dtype == F32
            body[:] = _residue_f32(v.reshape(-1, 3)).reshape(-1)
        elif e == "bfpatches":
            B, h, w, gh, gw = (a[k] for k in ("B", "h", "w", "gh", "gw"))
            CP = 3 * gh * gw
            rows = body.reshape(-1, CP)
            v = _norm_px_f32(a["rgb"].reshape(B, gh, h, gw, w, 3)).transpose(0, 2, 4, 5, 1, 3).reshape(-1, CP).astype(np.float16)
            keep = CP - CP % 8 if defect == "partial_chunk_missing" else CP
            rows[:, :keep] = v[:, :keep]
        else:
            assert e == "sam"
            src = R.sam_source(a).astype(F32)

            def axis(n_src, n_dst):
                if defect == "align_corners_coordinates":
                    s = np.arange(n_dst).astype(F32) * (F32(n_src - 1) / F32(max(n_dst - 1, 1)))
                else:
                    s = np.maximum((np.arange(n_dst).astype(F32) + F32(0.5)) * (F32(n_src) / F32(n_dst)) - F32(0.5), F32(0))
                i0 = np.minimum(s.astype(np.int64), n_src - 1)
                return i0, np.minimum(i0 + 1, n_src - 1), s - i0.astype(F32)
            x0, x1, wx = axis(a["sw"], a["dw"])
            y0, y1, wy = axis(a["sh"], a["dh"])
            wx, wy = wx[None, :], wy[:, None]
            v0 = (1 - wx) * src[y0][:, x0] + wx * src[y0][:, x1]
            v1 = (1 - wx) * src[y1][:, x0] + wx * src[y1][:, x1]
            v = (1 - wy) * v0 + wy * v1
            assert v.dtype == F32
            body[:] = (np.where(v > 0, 255, 0) if a["out_u8"] else v).reshape(-1)
    if defect == "stray_store_behind_the_buffer":
        buf[size - guard] = body[-1] if body[-1] != buf[size - guard] else 1
    return buf


def verdict(c, a, guard, got):
    """the GPU test's comparison on one buffer -> (rejected, violations)"""
    e = c["entry"]
    ref = R.evaluate(e, a, guard, got=got)
    first = R.initial_buffer(e, a, got.size)
    if got.dtype == np.uint8:
        v = R.u8_violations(got, ref, first)
    else:
        v = violations(got, ref, untouched=first)
    z = R.zero_bit_elements(e, a, got.size)
    v["nonzero_bits"] = int(np.ascontiguousarray(got).view({1: np.uint8, 2: np.uint16, 4: np.uint32}[got.dtype.itemsize])[z].astype(bool).sum())
    return rejected(v) or v["nonzero_bits"] > 0, v


def _reject(c, defect=None):
    a = args_of(c)
    guard = T.guard_of(c, a)
    return verdict(c, a, guard, emulate(c, a, guard, defect))


def test_emulations_are_inside_the_allowance_for_every_case():
    worst = defaultdict(float)
    for c in T.all_cases():
        bad, v = _reject(c)
        assert not bad, (c["id"], {k: v[k] for k in ("stray", "nonfinite", "outside", "ratio", "worst", "nonzero_bits")})
        worst[(c["entry"], c["kind"])] = max(worst[(c["entry"], c["kind"])], v["ratio"])
    print("\nlargest emulated error / allowance per entry and data kind:")
    for k, r in sorted(worst.items()):
        print(f"  {k[0]:10s} {k[1]:10s} {r:.3f}")
    assert all(worst[(e, k)] == 0 for e, k in worst if e in ("cls", "u8"))
    assert max(r for (e, _), r in worst.items() if e in ("patches", "tvpre", "bfpatches")) > 0.5  # no blanket: the f16 rounding alone comes close


DEFECTS = {  # defect -> the cases it is tried on
    "min_max_per_batch": lambda c: c["entry"] == "minmax" and c["B"] > 1 and c["n"] > 1 and c["kind"] in ("mixed", "negative", "huge"),
    "encoding_without_negative_branch": lambda c: c["entry"] == "minmax" and c["n"] > 1 and c["kind"] in ("mixed", "negative", "huge", "subnormal"),
    "tail_missing_in_the_reduction": lambda c: c["entry"] == "minmax" and c["kind"] == "mixed" and c["n"] >= 5 and c["n"] % 4,
    "normalisation_contracted": lambda c: c["entry"] == "minmax" and c["kind"] in ("mixed", "negative") and c["n"] >= 255,
    "rounding_not_truncation": lambda c: c["entry"] == "u8" and c["kind"] == "boundaries",
    "channel_order_ky_c_kx": lambda c: c["entry"] == "patches" and c["ps"] > 1 and c["kind"] == "random",
    "pad_columns_unwritten": lambda c: c["entry"] == "patches" and c["Kp"] > 3 * c["ps"] ** 2,
    "partial_chunk_missing": lambda c: c["entry"] == "bfpatches" and (3 * c["gw"] * c["gh"]) % 8,
    "cls_on_every_row": lambda c: c["entry"] == "cls" and c["T"] > 1,
    "align_corners_coordinates": lambda c: c["entry"] == "sam" and c["resize"] not in ("identity",),
    "first_pass_only": lambda c: c["entry"] in ("pre32", "head_out", "u8") and T.loops(c["B"] * c["H"] * c["W"] * 3 if c["entry"] == "pre32" else c["n"]),
    "stray_store_behind_the_buffer": lambda c: True,
}


def test_seeded_defects_are_rejected_by_the_comparison_the_gpu_test_uses():
    print()
    for defect, applies in DEFECTS.items():
        tried = [c for c in T.all_cases() if applies(c)]
        results = {c["id"]: _reject(c, defect) for c in tried}
        rejecting = [c for c in tried if results[c["id"]][0]]
        missed = [c["id"] for c in tried if c not in rejecting]
        print(f"{defect}: rejected by {len(rejecting)} of the {len(tried)} cases tried" + (": not by " + ", ".join(missed[:8]) + (" ..." if len(missed) > 8 else "") if missed else ""))
        assert rejecting and {c["entry"] for c in rejecting} == {c["entry"] for c in tried}, defect
        if defect == "align_corners_coordinates":  # every f32 output shows it; a thresholded one only where a sign moves with the coordinates
            assert all(T.case(m)["out_u8"] for m in missed) and len(missed) <= 2, missed
        if defect == "tail_missing_in_the_reduction":  # only where an extreme is planted in the tail of an aligned image can it show
            for c in tried:
                hit = any(T.image_aligned(b, c["n"]) and max(T.planted(c, b)) >= 4 * (c["n"] // 4) for b in range(c["B"]))
                assert (c in rejecting) == hit, c["id"]
            assert len(rejecting) >= 8
        if defect == "normalisation_contracted":  # the value at the minimum is the product's rounding error, not +0.0
            assert all(results[c["id"]][1]["nonzero_bits"] > 0 for c in rejecting) and len(rejecting) >= len(tried) // 2
        if defect == "stray_store_behind_the_buffer":
            for c in tried:
                v = results[c["id"]][1]
                assert v["stray"] == 1 and v["first_stray"] == args_size(c) and v["nonzero_bits"] == 0, c["id"]
        if defect in ("min_max_per_batch", "rounding_not_truncation", "channel_order_ky_c_kx", "pad_columns_unwritten", "partial_chunk_missing", "cls_on_every_row", "first_pass_only",
                      "stray_store_behind_the_buffer"):
            assert not missed, missed
        if defect == "first_pass_only":
            assert {c["entry"] for c in tried} == {"pre32", "head_out", "u8"}
        if defect == "encoding_without_negative_branch":  # every image with a negative value shows it
            assert not missed, missed


def args_size(c):
    a = args_of(c)
    return R.evaluate(c["entry"], a, T.guard_of(c, a))[0].size - T.guard_of(c, a)


def test_u8_twin_gives_the_buffer_comparison_verdicts():
    want = np.array([0, 255, 7, R.CANARY_U8, R.CANARY_U8], np.float64)
    ref = (want, np.zeros(5), np.array([True, True, True, False, False]))
    ok = np.array([0, 255, 7, R.CANARY_U8, R.CANARY_U8], np.uint8)
    assert not rejected(R.u8_violations(ok, ref, R.CANARY_U8))
    off = ok.copy()
    off[2] = 8
    v = R.u8_violations(off, ref, R.CANARY_U8)
    assert rejected(v) and v["outside"] == 1 and v["worst"] == 2 and v["stray"] == 0 and v["ratio"] == np.inf
    stray = ok.copy()
    stray[4] = 0
    v = R.u8_violations(stray, ref, R.CANARY_U8)
    assert rejected(v) and v["stray"] == 1 and v["first_stray"] == 4 and v["outside"] == 0
    with pytest.raises(AssertionError, match="1 bytes written that the call must leave alone, the first at 4"):
        R.assert_u8_buffer(stray, ref, "case", R.CANARY_U8)
    with pytest.raises(AssertionError, match="1 of 5 bytes differ"):
        R.assert_u8_buffer(off, ref, "case", R.CANARY_U8)


# ---- 4. the refusals ----------------------------------------------------------------------------------------------------------------------------

def test_refusal_tables_return_before_any_launch():
    """host code: every refusal is decided before the first HIP call, so the tables run without a device (the operands are one host buffer)"""
    names = {"patch size 0 and below": [("patches", dict(ps=0)), ("patches", dict(ps=-8))], "more images than the grid": [("patches", dict(B=65536)), ("minmax", dict(B=65536, n=1)), ("cls", dict(B=65536, T=1, C=1))],
             "null operands": [(e, dict(**{k: 0})) for e, ks in (("patches", ("rgb", "out", "mean", "inv")), ("pre32", ("rgb", "out", "mean", "inv")), ("cls", ("x", "cls", "pos")),
                                                                   ("head_out", ("x", "w", "depth")), ("minmax", ("depth", "out", "minmax")), ("u8", ("src", "dst"))) for k in ks],
             "empty extents": [("patches", dict(B=0)), ("patches", dict(H=0)), ("patches", dict(W=0)), ("pre32", dict(B=0)), ("cls", dict(T=0)), ("cls", dict(C=0)), ("head_out", dict(n=0)),
                               ("minmax", dict(n=0)), ("u8", dict(n=0)), ("u8", dict(n=-1))],
             "widths the head output has no kernel for": [("head_out", dict(C=C)) for C in (0, 12, 24, 48, 128)]}
    for what, entries in names.items():
        for entry, fields in entries:
            assert any(f == fields for f, _ in T.REFUSAL_TABLES[entry]), (what, entry, fields)
    assert set(T.REFUSAL_TABLES) == set(T.REFUSAL_BASES) == set(T.GROUPS) == set(T.ENTRY_POINT) and T.N_REFUSALS > 90
    misc = (CSRC / "kernels_misc.hip").read_text()
    m = re.search(r"int vx_preprocess_patches\(.*?\n\}", misc, re.S).group(0)
    assert m.index("ps > 0") < m.index("H % ps") and m.index("null operand") < m.index("H % ps") and m.index("B <= 65535") < m.index("hipLaunchKernelGGL")
    for name in ("vx_preprocess_f32", "vx_write_cls_rows", "vx_head_out_f32", "vx_minmax_normalize", "vx_f32_to_u8"):
        body = re.search(rf"int {name}\(.*?\n\}}", misc, re.S).group(0)
        assert body.index("VX_REQUIRE") < body.index("hipLaunchKernelGGL") and body.count("VX_REQUIRE") >= 2, name
    if L.get_lib().vx_device_count() > 0:
        return  # with a device the GPU suite runs the tables, on device memory (a refusal that regressed would launch on these host operands)
    scratch = np.zeros(T.REFUSAL_SCRATCH_BYTES, np.uint8)
    seen = []
    assert T.run_refusals(L.get_lib(), scratch.ctypes.data, scratch.ctypes.data, seen) == T.N_REFUSALS
    assert not scratch.any() and len(seen) == T.N_REFUSALS

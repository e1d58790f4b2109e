"""No device: the references of tests/stage_ref.py agree with what is already pinned to the reference project (tests/migan_ref.py,
tests/yolov9t_ref.py), migan_ref's upsample and downsample are themselves pinned on an asymmetric filter to plain loops over the header's
contract, the tables of tests/stage_cases.py span every shape, pointer combination, data kind and dispatch class, the data kinds are what they
claim, a float32 numpy emulation of each kernel's arithmetic in the kernel's tap order lies inside the allowance for EVERY case, emulations
with one seeded mistake each are rejected by the comparison the GPU test uses (buffer_check.violations and stage_ref.candidate_faults), the
three FIR mistakes pass again once the filter is symmetric, and the refusal tables return before any launch. No element and no case is exempt."""
import re
from collections import defaultdict
from pathlib import Path

import numpy as np
import pytest

import migan_ref
import stage_cases as T
import stage_ref as R
import yolov9t_ref
from buffer_check import rejected, violations
from visioncpp_amd import _lib as L

F32, F16 = np.float32, np.float16
CSRC = Path(__file__).resolve().parents[1] / "vision.cpp_amd" / "csrc"
_cache = {}


def args_of(c):
    if c["id"] not in _cache:
        _cache[c["id"]] = T.materialize(c)
    return _cache[c["id"]]


def torch_fir(f):
    """[4, 4, C] -> torch [C, 1, 4, 4]"""
    return np.ascontiguousarray(np.asarray(f, F32).transpose(2, 0, 1)[:, None])


def close32(got, want, scale=None):
    """to float32 accuracy: a few hundred u32 of the largest magnitude involved"""
    scale = np.abs(want).max() if scale is None else scale
    return np.abs(np.asarray(got, np.float64) - want).max() <= 512 * R.U32 * max(scale, 1.0)


# ---- 1. the references against what is already pinned -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cid", ["dw-2x5x7x64-normal", "dw-2x5x7x64-negative", "dw-1x4x6x128-normal"])
def test_depthwise_matches_migan_ref(cid):
    a = args_of(T.case(cid))
    pre, _ = R.dw_pre(a)
    got = migan_ref.depthwise(a["x"].astype(F32), torch_fir(a["w"]), a["bias"], 1, 1)
    assert close32(got, pre)
    assert close32(migan_ref.lrelu_agc(got), R.dw_act(a)[0])


@pytest.mark.parametrize("cid", ["dw_down-2x18x20x64-normal", "dw_down-1x6x34x128-normal", "dw_down-2x18x20x64-symmetric", "dw_down-1x2x2x64-normal"])
def test_down_matches_migan_ref_on_the_asymmetric_filter_too(cid):
    a = args_of(T.case(cid))
    act = migan_ref.lrelu_agc(migan_ref.depthwise(a["x"].astype(F32), torch_fir(a["w"]), a["bias"], 1, 1))
    assert close32(migan_ref.downsample(act, torch_fir(a["fir"])), R.dw_down(a)[0])


@pytest.mark.parametrize("cid", ["up-2x2x3x8-n1f1-normal", "up-1x5x9x24-n0f0-normal", "up-2x4x4x16-n1f1-symmetric", "up-1x1x1x8-n1f0-normal", "up-2x4x4x16-n0f1-normal"])
def test_upsample_matches_migan_ref_on_the_asymmetric_filter_too(cid):
    a = args_of(T.case(cid))
    got = migan_ref.upsample(a["y"].astype(F32), torch_fir(a["fir"]))
    if a["noise"] is not None:
        got = got + a["noise"][None, :, :, None]
    got = migan_ref.lrelu_agc(got)
    if a["feat"] is not None:
        got = got + a["feat"].astype(F32)
    assert close32(got, R.up(a)[0])


@pytest.mark.parametrize("cid", ["torgb-2x6x10x64-prev1-normal", "torgb-1x3x5x24-prev0-normal", "torgb-2x12x14x512-prev1-normal", "torgb-1x2x2x8-prev1-normal"])
def test_torgb_matches_migan_ref(cid):
    a = args_of(T.case(cid))
    got = migan_ref.conv1x1(a["x"].astype(F32), a["w"][:, :, None, None], a["bias"])
    if a["prev"] is not None:
        got = got + migan_ref.upsample(a["prev"], torch_fir(a["fir"]))
    want, allow = R.torgb(a)
    assert close32(got, want, (allow / R.U32).max() / 512)  # (in units of the sum of magnitudes: C terms)


def test_migan_ref_upsample_and_downsample_are_the_headers_contract_on_an_asymmetric_filter():
    """plain loops: zero insertion, 4x4 correlation at pad 2, crop; 4x4 at stride 2, pad 1"""
    rng = np.random.default_rng(5)
    h, w, C = 3, 5, 8
    x = rng.standard_normal((1, h, w, C)).astype(F32)
    f = T.fir_ref.asymmetric_fir(rng, C, 4.0).astype(F32)
    assert all(np.abs(v - f).max() > 0.05 for v in R.fir_variants(f).values())
    z = np.zeros((2 * h + 4, 2 * w + 4, C))
    for i in range(h):
        for j in range(w):
            z[2 + 2 * i, 2 + 2 * j] = x[0, i, j]
    up = np.zeros((2 * h, 2 * w, C))
    for Y in range(2 * h):
        for X in range(2 * w):
            for ky in range(4):
                for kx in range(4):
                    up[Y, X] += f[ky, kx].astype(np.float64) * z[Y + ky, X + kx]
    assert close32(migan_ref.upsample(x, torch_fir(f))[0], up)
    assert close32(T.fir_ref.upfirdn2x_raw(x, f)[0], up)
    H, W = 6, 10
    xd = rng.standard_normal((1, H, W, C)).astype(F32)
    p = np.zeros((H + 2, W + 2, C))
    p[1:-1, 1:-1] = xd[0]
    down = np.zeros((H // 2, W // 2, C))
    for oy in range(H // 2):
        for ox in range(W // 2):
            for ky in range(4):
                for kx in range(4):
                    down[oy, ox] += f[ky, kx].astype(np.float64) * p[2 * oy + ky, 2 * ox + kx]
    assert close32(migan_ref.downsample(xd, torch_fir(f))[0], down)
    assert close32(T.fir_ref.depthwise(xd, f, None, 2, 1)[0], down)


def test_yolo_references_match_yolov9t_ref():
    for c in T.group("avgpool2"):
        a = args_of(c)
        assert close32(yolov9t_ref.avg_pool2(a["x"][..., a["c0"]:a["c0"] + a["C"]].astype(F32)), R.avgpool2(a)[0])
    for c in T.group("spp"):
        a = args_of(c)
        C = a["C"]
        x = a["buf"][..., :C].astype(F32)
        assert not np.isnan(x).any() and not (np.signbit(x) & (x == 0)).any(), c["id"]  # no NaN, no -0.0: the maximum's bits are decided
        p1 = yolov9t_ref.max_pool5(x)
        p2 = yolov9t_ref.max_pool5(p1)
        p3 = yolov9t_ref.max_pool5(p2)
        want, written = R.spp(a)
        assert np.array_equal(want[..., C:4 * C], np.concatenate([p1, p2, p3], -1)) and np.array_equal(want[..., :C], x) and (want[..., 4 * C:] == R.CANARY).all()
        assert written[..., C:4 * C].all() and not written[..., :C].any() and not written[..., 4 * C:].any()
    for c in T.group("upsample2"):
        a = args_of(c)
        want, written = R.upsample2(a)
        assert np.array_equal(want[..., a["o0"]:a["o0"] + a["C"]], yolov9t_ref.upsample2(a["x"][..., a["c0"]:a["c0"] + a["C"]].astype(np.float64)))
        assert written.sum() == want[..., a["o0"]:a["o0"] + a["C"]].size
    for c in T.group("decode"):
        a = args_of(c)
        with np.errstate(over="ignore", under="ignore"):
            wb, ws = yolov9t_ref.decode([r.astype(F32) for r in a["raws"]])
        assert close32(wb, R.decode_boxes(a)[0]) and close32(ws, R.decode_scores(a)[0])


# ---- 2. the tables -------------------------------------------------------------------------------------------------------------------------------------

def test_tables_span_what_the_issue_names():
    g = T.group
    assert {c["shape"] for c in g("dw")} == {(1, 2, 2, 64), (2, 3, 5, 64), (2, 5, 7, 64), (1, 4, 6, 128)}
    assert {c["shape"] for c in g("dw_down")} == {(1, 2, 2, 64), (1, 16, 16, 64), (2, 18, 20, 64), (1, 6, 34, 128)}
    for e in ("dw", "dw_down", "up"):
        assert {c["kind"] for c in g(e)} == set(T.KINDS), e
    up = g("up")
    assert {c["shape"] for c in up} == {(1, 1, 1, 8), (2, 2, 3, 8), (1, 5, 9, 24), (2, 4, 4, 16)}
    for n in (0, 1):
        for f in (0, 1):
            assert len({c["shape"] for c in up if (c["noise"], c["feat"]) == (n, f)}) >= 2
    assert any(c["noise"] and c["shape"][0] == 2 for c in up)
    tg = g("torgb")
    assert {(c["shape"], c["prev"]) for c in tg} == {((1, 2, 2, 8), 1), ((1, 2, 2, 8), 0), ((1, 3, 5, 24), 0), ((2, 12, 14, 512), 1), ((2, 6, 10, 64), 1)}
    assert args_of(T.case("torgb-1x2x2x8-prev1-normal"))["prev"].shape == (1, 1, 1, 3)
    assert {(c["shape"], c["pix"], c["c0"]) for c in g("avgpool2")} == {((1, 2, 2, 8), 8, 0), ((2, 9, 12, 16), 40, 8), ((1, 3, 4, 24), 24, 0)}
    assert {c["shape"] for c in g("spp")} == {(1, 1, 1, 8, 32), (2, 3, 4, 8, 40), (1, 15, 15, 8, 32), (2, 9, 12, 16, 72)} and {c["kind"] for c in g("spp")} == {"normal", "negative", "lowest"}
    assert {(c["shape"], c["x_pix"], c["c0"], c["y_pix"], c["o0"]) for c in g("upsample2")} == {((1, 1, 1, 8), 8, 0, 8, 0), ((2, 3, 5, 16), 40, 8, 24, 8)}
    dc = g("decode")
    assert {(c["shape"], c["conf"], c["cand"]) for c in dc} == {(s, conf, 1) for s in ((1, 32, 8), (2, 64, 16), (3, 96, 8), (1, 64, 80)) for conf in (0.25, 0.0, 1.5)} | {(s, 0.25, 0) for s in T.DECODE_SHAPES}
    assert R.n_anchors(32) == 21 and 4 + 8 // 8 == 5 and 4 + 80 // 8 == 14 and R.grids(96) == (12, 6, 3) and (3 * R.n_anchors(96) * 5) % 64 and (3 * R.n_anchors(96) * 5) % 256
    for e in R.FIR_ENTRIES:  # every FIR case is asymmetric but the one that keeps the trained file's filter
        assert [c["fir"] for c in g(e)].count("symmetric") == 1 and all(c["kind"] == "normal" for c in g(e) if c["fir"] == "symmetric")


def test_every_dispatch_class_is_hit_and_the_restated_arithmetic_is_the_sources():
    mig, yolo = (CSRC / "kernels_migan.hip").read_text(), (CSRC / "kernels_yolov9t.hip").read_text()
    assert "constexpr int DT = 8, DS = 2 * DT + 2, DC = 32;" in mig and (T.DT, T.DC) == (8, 32)
    assert "const dim3 grid((unsigned)(C / DC), (unsigned)(((OH + DT - 1) / DT) * ((OW + DT - 1) / DT)), (unsigned)B);" in mig
    assert "const int J = 4 + nc / 8;" in yolo and "const long i = valid ? i0 : total - 1;" in yolo and "if (__all(n == 0 || b == b_first))" in yolo
    assert "__shared__ float sw[3 * 512];" in mig
    grids = {c["id"]: T.down_grid(*c["shape"]) for c in T.group("dw_down")}
    assert grids["dw_down-1x2x2x64-normal"] == (2, 1, 1, 1) and grids["dw_down-1x16x16x64-normal"] == (2, 1, 1, 1) and grids["dw_down-2x18x20x64-normal"] == (2, 2, 2, 2)
    assert grids["dw_down-1x6x34x128-normal"] == (4, 1, 3, 1) and (18 // 2 % 8, 20 // 2 % 8) == (1, 2)
    assert {T.blocks(np.prod(c["shape"]) // 8) > 1 for c in T.group("dw")} == {True, False} and (2 * 5 * 7 * 8) % 256
    assert {T.blocks(np.prod(c["shape"]) * 4 // 8) > 1 for c in T.group("up")} == {True, False} and (10 * 18 * 3) % 256
    assert {(c["noise"], c["feat"]) for c in T.group("up")} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert {c["prev"] for c in T.group("torgb")} == {0, 1} and T.blocks(2 * 12 * 14) == 2 and max(c["shape"][3] for c in T.group("torgb")) == 512
    paths = defaultdict(int)
    for c in T.group("decode"):
        a = args_of(c)
        assert R.undecided(a) == 0, c["id"]  # no class score within its allowance of conf: the candidate set equals the reference's
        total, straddle, per_lane, first_side, other_side = T.decode_waves(a)
        n = sum(len(v) for v in R.reference_candidates(a))
        A = R.n_anchors(a["S"])
        assert n == total.sum() and n == {0.25: n, 0.0: a["B"] * A * a["nc"], 1.5: 0}[c["conf"]]
        if c["conf"] == 0.25:
            assert 0 < n < a["B"] * A * a["nc"] and (total == 0).any(), c["id"]  # at least one wave without a candidate
            paths["uniform"] += int((~per_lane & (total > 0)).sum())
            paths["per_lane"] += int(per_lane.sum())
            paths["both_sides"] += int((straddle & (first_side > 0) & (other_side > 0)).sum())
        paths["dense" if not c["cand"] else "list"] += 1
    assert all(paths[k] > 0 for k in ("uniform", "per_lane", "both_sides", "dense", "list")), dict(paths)


def test_data_kinds_are_what_they_claim():
    for e in ("dw", "dw_down", "up"):
        for c in T.group(e):
            a = args_of(c)
            share, neg = R.clamp_share(e, a), R.negative_share(e, a)
            if c["kind"] == "spikes":
                assert 0.01 <= share <= 0.5, (c["id"], share)
            elif c["kind"] == "negative":
                assert neg >= 0.8, (c["id"], neg)
            elif c["kind"] == "normal":
                assert share == 0 and 0.1 < neg < 0.9, (c["id"], share, neg)
            else:
                src = a["x"] if e != "up" else a["y"]
                assert (np.abs(src) == 65504).any() and ((src != 0) & (np.abs(src.astype(np.float64)) < 2.0 ** -14)).any() and share > 0, c["id"]
    for c in T.group("spp"):
        x = args_of(c)["buf"][..., :c["shape"][3]]
        assert {"negative": (x < 0).all(), "lowest": (x == -65504).all(), "normal": (x > 0).any() and (x < 0).any() or x.size == 8}[c["kind"]], c["id"]
    for c in T.group("avgpool2"):
        if c["kind"] == "edges":
            want, _ = R.avgpool2(args_of(c))
            assert want[0, 0, 0, 0] == 65504.0 and np.isfinite(want.astype(F16)).all()
    one_hot = set()
    for c in T.group("decode"):
        a = args_of(c)
        d = np.concatenate([r.reshape(a["B"], -1, 64 + a["nc"])[..., :64].reshape(a["B"], -1, 4, 16) for r in a["raws"]], 1).astype(np.float64)
        cls = np.concatenate([r.reshape(a["B"], -1, 64 + a["nc"])[..., 64:] for r in a["raws"]], 1)
        assert (cls == 65504).any() and (cls == -65504).any()
        s, e = R.decode_scores(a)
        assert (s[cls == 65504] == 1).all() and (s[cls == -65504] == 0).all() and (e[cls == -65504] == 0).all()
        hot = (d.max(-1) - np.sort(d, -1)[..., -2]) >= 60
        one_hot |= set(d.argmax(-1)[hot].tolist())
        boxes, _ = R.decode_boxes(a)
        equal = np.ptp(d, axis=-1) == 0
        assert equal.any() and hot.any() and (np.abs(d[hot]).max() == 65504)
        side = np.concatenate([np.full(g * g, 8.0 * 2 ** lv) for lv, g in enumerate(R.grids(a["S"]))])[None, :, None]
        dist = np.abs(boxes / side - np.round(boxes / side * 2) / 2)  # the distance from the anchor (x.5) is the expectation
        assert (dist[equal] < 1e-12).all()  # 7.5 from an x.5 anchor: an integer
    assert {0, 15} <= one_hot and len(one_hot) >= 8


def test_the_canary_is_no_value_a_call_writes_and_the_decode_allowances_stay_under_the_ceiling():
    n = 0
    for c in T.all_cases():
        a = args_of(c)
        for part in (("boxes", "scores") if c["entry"] == "decode" else (None,)):
            want, allow, written = R.evaluate(c["entry"], a, T.GUARD, part)
            assert np.isfinite(want).all() and np.isfinite(allow).all() and (allow >= 0).all(), c["id"]
            assert (np.abs(want - R.CANARY) > allow + 1000)[written].all(), c["id"]
            first = R.initial_buffer(c["entry"], a, want.size, part).astype(np.float64)
            assert not written[-T.GUARD:].any() and np.array_equal(want[~written], first[~written]) and (first[-T.GUARD:] == R.CANARY).all() and not allow[~written].any()
            assert T.GUARD >= R.min_guard(c["entry"]) >= 2048
            if c["entry"] in ("spp", "upsample2"):
                assert not allow.any() and 0 < written.sum() < written.size - T.GUARD + (c["shape"][:3] == (1, 1, 1) and c["entry"] == "upsample2")
            else:
                assert written[:-T.GUARD].all()
            if part == "scores":
                assert allow.max() < R.SCORE_CEILING, (c["id"], allow.max())
            if part == "boxes":
                assert allow.max() < R.BOX_CEILING_PER_S * a["S"], (c["id"], allow.max())
            if R.out_dtype(c["entry"]) == F16:
                assert np.isfinite(want[written].astype(F16)).all(), c["id"]
            n += 1
    assert n == len(T.all_cases()) + len(T.group("decode")) > 80


def test_every_fir_case_shows_a_flipped_and_a_transposed_filter_in_every_channel():
    """the filter differs from its own flip and its own transpose by more than 100 times the case's largest allowance, in every channel. Both sides
    in their own scale: a tap that moves by the share d of the largest tap moves an output by about d times its size, so the largest tap difference
    over the largest tap of the channel is held against the largest allowance over the largest |want| of the case. On the output itself the changed
    filter lies more than 100 allowances away somewhere in every case; the symmetric filter shows neither change anywhere. Where the absolute form
    can hold -- the `normal` cases of torgb (an f32 output) and of the upsample without feat (outputs of order 1) -- it is asserted as stated: the
    largest tap difference of every channel exceeds 100 times the case's largest allowance. Next to the clamp an allowance is up to 0.125, next to
    a feat of order 3 about 0.0024: 100 of those are more than any tap (the largest is 0.7)"""
    fn = {"dw_down": R.dw_down, "up": R.up, "torgb": R.torgb}
    n = literal = 0
    for e in R.FIR_ENTRIES:
        for c in T.group(e):
            a = args_of(c)
            if e == "torgb" and a["prev"] is None:
                continue
            want, allow = fn[e](a)
            f = a["fir"].astype(np.float64)
            for name in ("flipped", "transposed"):
                g = R.fir_variants(f)[name]
                other, _ = fn[e](a, fir=g.astype(F32))
                if c["fir"] == "symmetric":
                    assert np.array_equal(f, g) and np.array_equal(other, want), (c["id"], name)
                    continue
                tap_share = np.abs(f - g).max((0, 1)) / np.abs(f).max((0, 1))
                assert (tap_share > 100 * allow.max() / np.abs(want).max()).all(), (c["id"], name, tap_share.min(), allow.max() / np.abs(want).max())
                assert (np.abs(other - want) / np.maximum(allow, R.TINY16)).max() > 100, (c["id"], name)
                if c["kind"] == "normal" and (e == "torgb" or (e == "up" and not c["feat"])):  # the absolute form, where taps of at most 0.7 can meet it
                    assert (np.abs(f - g).max((0, 1)) > 100 * allow.max()).all(), (c["id"], name, np.abs(f - g).max((0, 1)).min(), allow.max())
                    literal += 1
                n += 1
    assert n >= 50 and literal == 2 * (8 + 3)


# ---- 3. float32 emulations of the kernels, with the defects they can carry --------------------------------------------------------------------------

def agc32(v, defect=None):
    v = v.astype(F32)
    t = np.where(v > 0, F32(0.2) * v, v) if defect == "slope_on_positives" else np.where(v < 0, F32(0.2) * v, v)
    g = t * F32(1.41421356)
    assert g.dtype == F32
    edge = F32(255.875) if defect == "clamp_one_f16_step_low" else F32(256)
    return g if defect == "clamp_missing" else np.clip(g, -edge, edge)


def dw32(a, defect=None):
    x, w = a["x"].astype(F32), a["w"].astype(F32)
    B, H, W, C = x.shape
    p = np.zeros((B, H + 2, W + 2, C), F32)
    p[:, 1:-1, 1:-1] = x
    acc = np.broadcast_to(a["bias"].astype(F32), x.shape).copy()
    for ky in range(3):
        for kx in range(3):
            acc = acc + p[:, ky:ky + H, kx:kx + W] * w[ky, kx]
    assert acc.dtype == F32
    return agc32(acc, defect)


def tap(fir, ky, kx, py, px, defect):
    """the FIR tap a kernel pairs with (ky, kx) at output parity (py, px)"""
    if defect == "fir_flipped":
        ky, kx = 3 - ky, 3 - kx
    elif defect == "fir_transposed":
        ky, kx = kx, ky
    elif defect == "fir_parity_swapped":  # even outputs take taps 3 and 1 where 0 and 2 belong
        ky, kx = (3 - ky if py == 0 else ky), (3 - kx if px == 0 else kx)
    return fir[ky, kx]


def down32(a, defect=None):
    act = dw32(a, defect)
    if defect == "f16_between":
        act = act.astype(F16).astype(F32)
    B, H, W, C = act.shape
    OH, OW = H // 2, W // 2
    fir = a["fir"][..., np.arange(C) % T.DC] if defect == "channel_block_dropped" else a["fir"]
    out = np.zeros((B, OH, OW, C), F32)
    for ty0 in range(0, OH, T.DT):
        for tx0 in range(0, OW, T.DT):
            s = np.zeros((B, 18, 18, C), F32)
            for fy in range(18):
                for fx in range(18):
                    Y, X = 2 * ty0 - 1 + fy, 2 * tx0 - 1 + fx
                    if defect == "halo_off_by_one" and fx == 0 and tx0 > 0:
                        X -= 1
                    if 0 <= Y < H and 0 <= X < W:
                        s[:, fy, fx] = act[:, Y, X]
            nh, nw = min(T.DT, OH - ty0), min(T.DT, OW - tx0)
            acc = np.zeros((B, nh, nw, C), F32)
            for ky in range(4):
                for kx in range(4):
                    acc = acc + s[:, ky:ky + 2 * nh:2, kx:kx + 2 * nw:2] * tap(fir, ky, kx, 1, 1, defect)
            out[:, ty0:ty0 + nh, tx0:tx0 + nw] = acc
    assert out.dtype == F32
    return out


def poly32(x, fir, defect, full_extent=False):
    """the polyphase x2 FIR of x f32 [B, h, w, C] as both kernels index it -> f32 [B, 2h, 2w, C]; full_extent: the source indexed as if it had the output's extent"""
    B, h, w, C = x.shape
    flat = x.reshape(-1, C)
    hh, ww = (2 * h, 2 * w) if full_extent else (h, w)
    out = np.zeros((B, 2 * h, 2 * w, C), F32)
    Y, X = np.meshgrid(np.arange(2 * h), np.arange(2 * w), indexing="ij")
    py, px, my, mx = Y & 1, X & 1, Y >> 1, X >> 1
    for b in range(B):
        for ty in range(2):
            for tx in range(2):
                iy, ix = my - 1 + py + ty, mx - 1 + px + tx
                ok = (iy >= 0) & (iy < hh) & (ix >= 0) & (ix < ww)
                src = flat[((b * hh + iy) * ww + ix) % flat.shape[0]]
                f = np.zeros((2 * h, 2 * w, C), F32)
                for qy in range(2):
                    for qx in range(2):
                        f[qy::2, qx::2] = tap(fir, qy + 2 * ty, qx + 2 * tx, qy, qx, defect)
                out[b] = out[b] + np.where(ok[..., None], src * f, F32(0))
    assert out.dtype == F32
    return out


def up32(a, defect=None):
    B, h, w, C = a["y"].shape
    acc = poly32(a["y"].astype(F32), a["fir"], defect)
    nz = np.zeros((B, 2 * h, 2 * w), F32)
    if a["noise"] is not None:
        for b in range(B):
            nz[b] = np.roll(a["noise"].reshape(-1), -b).reshape(2 * h, 2 * w) if defect == "noise_per_image" else a["noise"]
    nz = nz[..., None]
    fv = a["feat"].astype(F32) if a["feat"] is not None and defect != "feat_dropped" else F32(0)
    out = agc32(acc, defect) + nz + fv if defect == "noise_after_activation" else agc32(acc + nz, defect) + fv
    assert out.dtype == F32
    return out


def torgb32(a, defect=None):
    x = a["x"].astype(F32)
    w = a["w"][[1, 0, 2]] if defect == "weight_rows_swapped" else a["w"]
    o = np.broadcast_to(a["bias"], x.shape[:3] + (3,)).astype(F32)
    for ch in range(x.shape[-1]):
        o = o + x[..., ch:ch + 1] * w[:, ch]
    if a["prev"] is not None:
        o = o + poly32(a["prev"], a["fir"], defect, full_extent=defect == "prev_full_extent")
    assert o.dtype == F32
    return o


def avgpool32(a, defect=None):
    x = a["x"].astype(F32)[..., a["c0"]:a["c0"] + a["C"]]
    d = x[:, 1:, :-1] if defect == "avgpool_column_w" else x[:, 1:, 1:]
    return (((x[:, :-1, :-1] + x[:, :-1, 1:]) + x[:, 1:, :-1]) + d) * F32(0.25)


def spp16(a, defect=None):
    C = a["C"]
    out = a["buf"].copy()
    x = a["buf"][..., :C].astype(np.float64)
    radii = (2, 3, 6) if defect == "spp_ring_radius" else (2, 4, 6)
    planes = [R.window_max(x, r, 0.0 if defect == "spp_zero_padding" else -np.inf) for r in radii]
    if defect == "spp_planes_swapped":
        planes = [planes[0], planes[2], planes[1]]
    out[..., C:4 * C] = np.concatenate(planes, -1)
    return out


def upsample2_16(a, defect=None):
    x = a["x"][..., a["c0"]:a["c0"] + a["C"]]
    B, h, w, _ = x.shape
    out = np.full((B, 2 * h, 2 * w, a["y_pix"]), R.CANARY, F16)
    iy, ix = np.arange(2 * h) >> 1, np.arange(2 * w) >> 1
    if defect == "upsample2_rounds_up":
        iy, ix = np.minimum((np.arange(2 * h) + 1) >> 1, h - 1), np.minimum((np.arange(2 * w) + 1) >> 1, w - 1)
    out[..., a["o0"]:a["o0"] + a["C"]] = x[:, iy][:, :, ix] + (F16(0.0) if defect == "upsample2_zero_sign_lost" else x[:, iy][:, :, ix] * F16(0.0))
    return out


def decode32(a, defect=None):
    """-> boxes f32 [B, A, 4], scores f32 [B, A, nc]"""
    boxes, scores = [], []
    with np.errstate(over="ignore", under="ignore"):
        for lv, r in enumerate(a["raws"]):
            B, g, _, ch = r.shape
            stride = F32(8.0 * 2 ** (0 if defect == "decode_wrong_stride" and lv == 1 else lv))
            v = r.astype(F32).reshape(B, g * g, ch)
            d = v[..., :64].reshape(B, g * g, 4, 16)
            e = np.exp(d - d.max(-1, keepdims=True))
            s, ws = np.zeros(e.shape[:-1], F32), np.zeros(e.shape[:-1], F32)
            for k in range(16):
                s = s + e[..., k]
                ws = ws + e[..., k] * F32(k + 1 if defect == "decode_bins_from_one" else k)
            dist = ws / s
            cell = np.arange(g * g)
            ax, ay = (cell % g).astype(F32) + F32(0.5), (cell // g).astype(F32) + F32(0.5)
            if defect == "decode_anchors_swapped":
                ax, ay = ay, ax
            anc = np.stack([ax, ay, ax, ay], -1)[None]
            sign = np.array([-1, 1 if defect == "decode_side_sign" else -1, 1, 1], F32)
            out = (anc + sign * dist) * stride
            assert out.dtype == F32 and e.dtype == F32
            boxes.append(out)
            scores.append(F32(1) / (F32(1) + np.exp(-v[..., 64:])))
    return np.concatenate(boxes, 1), np.concatenate(scores, 1)


DENSE = {"dw": dw32, "dw_down": down32, "up": up32, "torgb": torgb32, "avgpool2": avgpool32, "spp": spp16, "upsample2": upsample2_16}


def _buffer(c, a, values, part=None):
    size = R.evaluate(c["entry"], a, T.GUARD, part)[0].size
    buf = R.initial_buffer(c["entry"], a, size, part)
    with np.errstate(over="ignore"):
        buf[:size - T.GUARD] = np.asarray(values).reshape(-1)
    return buf


def emulate(c, a, defect=None):
    """-> the buffers the call leaves, as the GPU test reads them back: {part: flat buffer with its guard}"""
    if c["entry"] != "decode":
        bufs = {None: _buffer(c, a, DENSE[c["entry"]](a, defect))}
    else:
        boxes, scores = decode32(a, defect)
        bufs = {"boxes": _buffer(c, a, boxes, "boxes"), "scores": _buffer(c, a, scores, "scores")}
        if a["cand"]:
            B, A, nc = scores.shape
            count = np.full(B + T.COUNT_GUARD, R.CANARY_I32, np.int32)
            idx, score = np.full(B * A * nc + T.GUARD, R.CANARY_I32, np.int32), np.full(B * A * nc + T.GUARD, R.CANARY, F32)
            for b in range(B):
                k = np.flatnonzero(scores[b].ravel() >= F32(a["conf"]))[::-1]  # (any order)
                if defect == "candidate_duplicated" and k.size > 1:
                    k = np.concatenate([k[:1], k[:-1]])
                if defect == "candidate_missing" and k.size:
                    k = k[:-1]
                lo = (0 if defect == "candidate_wrong_region" else b) * A * nc
                idx[lo:lo + k.size], score[lo:lo + k.size] = k, scores[b].ravel()[k]
                count[b] = k.size + (defect == "count_off_by_one")
            bufs.update(count=count, idx=idx, score=score)
    if defect == "stray_store_behind_the_buffer":
        for part in (None, "boxes", "scores"):
            if part in bufs:
                bufs[part][-T.GUARD] = 1.0
    return bufs


def verdict(c, a, bufs):
    """the GPU test's comparison -> (rejected, {part: violations}, candidate faults)"""
    bad, vs, faults = False, {}, []
    for part in (("boxes", "scores") if c["entry"] == "decode" else (None,)):
        got = bufs[part]
        v = violations(got, R.evaluate(c["entry"], a, T.GUARD, part), untouched=R.initial_buffer(c["entry"], a, got.size, part))
        vs[part] = v
        bad |= rejected(v)
        if c["entry"] in ("spp", "upsample2"):
            bad |= R.bit_faults(got, R.evaluate(c["entry"], a, T.GUARD, part)) > 0
    if c["entry"] == "decode" and a["cand"]:
        B, nc = a["B"], a["nc"]
        faults = R.candidate_faults(a, bufs["scores"][:-T.GUARD].reshape(B, -1, nc), bufs["count"], bufs["idx"], bufs["score"], T.GUARD)
        got_sets = [np.sort(bufs["idx"][b * bufs["scores"][:-T.GUARD].size // B:][:max(int(bufs["count"][b]), 0)]) for b in range(B)]
        if not faults and not all(np.array_equal(g, w) for g, w in zip(got_sets, R.reference_candidates(a))):
            faults = ["the candidate set is not the float64 reference's"]
    return bad or bool(faults), vs, faults


def _reject(c, defect=None):
    a = args_of(c)
    return verdict(c, a, emulate(c, a, defect))


def test_emulations_are_inside_the_allowance_for_every_case():
    worst = defaultdict(float)
    for c in T.all_cases():
        bad, vs, faults = _reject(c)
        assert not bad, (c["id"], faults, {p: {k: v[k] for k in ("stray", "nonfinite", "outside", "ratio", "worst")} for p, v in vs.items()})
        for part, v in vs.items():
            worst[(c["entry"] + ("/" + part if part else ""), c["kind"])] = max(worst[(c["entry"] + ("/" + part if part else ""), c["kind"])], v["ratio"])
    print("\nlargest emulated error / allowance per entry and data kind:")
    for k, r in sorted(worst.items()):
        print(f"  {k[0]:16s} {k[1]:10s} {r:.3f}")
    assert all(r == 0 for (e, _), r in worst.items() if e in ("spp", "upsample2"))
    assert max(r for (e, _), r in worst.items() if e in ("dw", "dw_down", "up", "avgpool2")) > 0.4  # no blanket: the f16 rounding alone comes close


FIR_DEFECTS = ("fir_flipped", "fir_transposed", "fir_parity_swapped")


def _fir_case(c):
    return c["entry"] in R.FIR_ENTRIES and c["fir"] == "asymmetric" and (c["entry"] != "torgb" or c["prev"])


DEFECTS = {  # defect -> the cases it is tried on
    "fir_flipped": _fir_case,
    "fir_transposed": _fir_case,
    "fir_parity_swapped": lambda c: _fir_case(c) and c["entry"] != "dw_down",
    "noise_per_image": lambda c: c["entry"] == "up" and c["noise"] and c["shape"][0] > 1,
    "noise_after_activation": lambda c: c["entry"] == "up" and c["noise"],
    "feat_dropped": lambda c: c["entry"] == "up" and c["feat"],
    "clamp_missing": lambda c: c["entry"] in ("dw", "dw_down", "up") and c["kind"] == "spikes",
    "clamp_one_f16_step_low": lambda c: c["entry"] in ("dw", "up") and c["kind"] == "spikes",
    "slope_on_positives": lambda c: c["entry"] in ("dw", "dw_down", "up"),
    "f16_between": lambda c: c["entry"] == "dw_down" and c["kind"] == "normal",
    "halo_off_by_one": lambda c: c["entry"] == "dw_down" and T.down_grid(*c["shape"])[2] > 1,
    "channel_block_dropped": lambda c: c["entry"] == "dw_down",
    "weight_rows_swapped": lambda c: c["entry"] == "torgb",
    "prev_full_extent": lambda c: c["entry"] == "torgb" and c["prev"] and c["shape"][1] > 2,
    "avgpool_column_w": lambda c: c["entry"] == "avgpool2",
    "spp_ring_radius": lambda c: c["entry"] == "spp" and c["kind"] != "lowest" and c["shape"][1] > 3,
    "spp_zero_padding": lambda c: c["entry"] == "spp" and c["kind"] in ("negative", "lowest"),
    "spp_planes_swapped": lambda c: c["entry"] == "spp" and c["kind"] != "lowest" and c["shape"][1] > 4,
    "upsample2_rounds_up": lambda c: c["entry"] == "upsample2" and c["shape"][1] > 1,
    "upsample2_zero_sign_lost": lambda c: c["entry"] == "upsample2" and c["kind"] == "edges" and c["shape"][1] > 1,
    "decode_anchors_swapped": lambda c: c["entry"] == "decode",
    "decode_wrong_stride": lambda c: c["entry"] == "decode",
    "decode_side_sign": lambda c: c["entry"] == "decode",
    "decode_bins_from_one": lambda c: c["entry"] == "decode",
    "candidate_duplicated": lambda c: c["entry"] == "decode" and c["cand"] and c["conf"] < 1,
    "candidate_missing": lambda c: c["entry"] == "decode" and c["cand"] and c["conf"] < 1,
    "candidate_wrong_region": lambda c: c["entry"] == "decode" and c["cand"] and c["conf"] < 1 and c["shape"][0] > 1,
    "count_off_by_one": lambda c: c["entry"] == "decode" and c["cand"],
    "stray_store_behind_the_buffer": lambda c: True,
}


def test_seeded_defects_are_rejected_by_the_comparison_the_gpu_test_uses():
    print()
    for defect, applies in DEFECTS.items():
        tried = [c for c in T.all_cases() if applies(c)]
        assert tried, defect
        rejecting = [c for c in tried if _reject(c, defect)[0]]
        missed = [c["id"] for c in tried if c not in rejecting]
        print(f"{defect}: rejected by {len(rejecting)} of the {len(tried)} cases tried" + (": not by " + ", ".join(missed[:8]) if missed else ""))
        assert not missed, (defect, missed)


def test_the_fir_defects_pass_once_the_filter_is_symmetric():
    """why the asymmetric cases exist: on the trained file's filter a kernel that flips, transposes or mispairs its taps is inside every allowance"""
    symmetric = [c for c in T.all_cases() if c["entry"] in R.FIR_ENTRIES and c["fir"] == "symmetric"]
    assert {c["entry"] for c in symmetric} == set(R.FIR_ENTRIES)
    for c in symmetric:
        twin = T.case(c["id"].replace("symmetric", "normal"))
        assert twin["shape"] == c["shape"] and twin["fir"] == "asymmetric"
        for defect in FIR_DEFECTS:
            if defect == "fir_parity_swapped" and c["entry"] == "dw_down":
                continue
            assert not _reject(c, defect)[0], (c["id"], defect)
            assert _reject(twin, defect)[0], (twin["id"], defect)


# ---- 4. the refusals ----------------------------------------------------------------------------------------------------------------------------------

def _clause(text):
    """one operand of a VX_REQUIRE condition's && / || chain, without the parentheses that belong to the chain"""
    t = text.strip().rstrip(",").strip()  # (the last operand carries the comma before the message)
    while t.startswith("(") and t.count("(") > t.count(")"):
        t = t[1:].strip()
    while t.endswith(")") and t.count(")") > t.count("("):
        t = t[:-1].strip()
    return t


def test_refusal_tables_return_before_any_launch():
    """host code: every refusal is decided before the first HIP call, so the tables run without a device (the operands are one host buffer); one row
    per clause of every VX_REQUIRE"""
    assert set(T.REFUSAL_TABLES) == set(T.REFUSAL_BASES) and T.N_REFUSALS > 100
    mig, yolo = (CSRC / "kernels_migan.hip").read_text(), (CSRC / "kernels_yolov9t.hip").read_text()
    for name, src, table in (("vx_migan_dwconv_f16", mig, "dw"), ("vx_migan_upsample_f16", mig, "up"), ("vx_migan_torgb", mig, "torgb"), ("vx_migan_preprocess", mig, "preprocess"),
                             ("vx_yolo_avgpool2_f16", yolo, "avgpool2"), ("vx_yolo_spp_f16", yolo, "spp"), ("vx_yolo_upsample2_f16", yolo, "upsample2"), ("vx_yolo_decode", yolo, "decode")):
        body = re.search(rf"int {name}\(.*?\n\}}", src, re.S).group(0)
        requires = re.findall(r"VX_REQUIRE\((.*?)\"", body, re.S)
        clauses = [_clause(t) for r in requires for t in re.split(r"&&|\|\|", r)]
        assert body.rindex("VX_REQUIRE") < body.index("hipLaunchKernelGGL(", body.rindex("VX_REQUIRE"))
        assert clauses == list(T.CLAUSE_ROWS[table]), (name, clauses)  # every clause of the source, in its order, names a row ...
        rows = [f for f, _ in T.REFUSAL_TABLES[table]]
        assert all(f in rows for f in T.CLAUSE_ROWS[table].values()), name  # ... and that row is in the table
        if "migan" in name:
            assert "aligned16(" in body and any("16-byte aligned" in m for _, m in T.REFUSAL_TABLES[table]), name
    if L.get_lib().vx_device_count() > 0:
        return  # with a device the GPU suite runs the tables, on device memory (a refusal that regressed would launch on these host operands)
    scratch = np.zeros(T.REFUSAL_SCRATCH_BYTES, np.uint8)
    seen = []
    assert T.run_refusals(L.get_lib(), scratch.ctypes.data, seen) == T.N_REFUSALS
    assert not scratch.any() and len(seen) == T.N_REFUSALS

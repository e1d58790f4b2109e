"""No device: the references of tests/rows_ref.py agree with the CPU oracle and the older numpy references, the tables of tests/rows_cases.py
cover every dispatch class of every launcher, a float32 numpy emulation of the LayerNorm kernels' arithmetic (two-pass, per-lane partial sums,
tree reduction) lies inside the allowance for EVERY LayerNorm case in two summation orders, and emulations with one seeded mistake each are
rejected by the comparison the GPU test uses (buffer_check.violations). No element and no case is exempt anywhere in this file."""
import re
from collections import defaultdict
from pathlib import Path

import numpy as np
import pytest

import dwconv_ref
import rows_cases as T
import rows_ref as R
import window_ref
from buffer_check import rejected, violations
from oracle import oracle
from visioncpp_amd import _lib as L

F32 = np.float32
LN_GROUPS = R.LAYER_NORMS


def _ln_cases():
    return [c for g in LN_GROUPS for c in T.group(g)]


def _width(c):
    return 4 * c["C"] if c["entry"] == "swin_merge" else c["C"]


# ---- 1. the references against the oracle and the older references ------------------------------------------------------------------------

ORACLE_SAMPLE = ["ln32-c128-m5", "ln32-c65-m131", "ln32-c200-m4", "tvln-c136-res9ws4-f16", "tvln-c264-rows-f32", "swinln-c136-5x13-ws4s1", "swinln-c8-14x21-ws7s3",
                 "swinlds-c136-ld144-f16", "merge-c40-4x6", "merge-c64-6x10"]


@pytest.mark.parametrize("cid", ORACLE_SAMPLE)
def test_layer_norm_reference_matches_the_oracle(cid):
    """Bound 2e-5 of the largest value: the oracle's f32 statistics carry (C + 8) u32 = 1.6e-5 in the worst case at the widths sampled (<= 264)."""
    c = T.case(cid)
    a = T.materialize(c)
    x, pad = R.layer_norm_source(c["entry"], a)
    want = R.layer_norm_entry(c["entry"], a)[0]
    got = oracle.layer_norm(x[~pad], a["w"], a["b"], a["eps"])
    assert _width(c) <= 264 and np.abs(got - want[~pad]).max() < 2e-5 * np.abs(want).max()


def test_window_maps_match_the_older_references():
    rng = np.random.default_rng(1)
    for H, W in T.SWIN_MAPS:
        for ws, shift in T.SWIN_WINDOWS:
            x = rng.standard_normal((2, H, W, 3))
            src = R.partition_rows(2, H, W, ws, shift)
            rows, valid = window_ref.windows(x, ws, shift)
            np.testing.assert_array_equal(valid, src >= 0)
            np.testing.assert_array_equal(rows[valid], x.reshape(-1, 3)[src[valid]])
            assert not rows[~valid].any() and sorted(src[src >= 0].tolist()) == list(range(2 * H * W))
            back = R.reverse_rows(2, H, W, ws, shift)
            np.testing.assert_array_equal(src[back], np.arange(2 * H * W))  # reverse undoes partition, and lands on no pad row
    for res, ws in T.TV_WINDOWS:
        x = rng.standard_normal((2, res, res, 3))
        win, padded = dwconv_ref.window_partition(x, ws)
        src = R.partition_rows(2, res, res, ws)
        np.testing.assert_array_equal(np.where((src < 0)[:, None], 0.0, x.reshape(-1, 3)[np.maximum(src, 0)]), win.reshape(-1, 3))
        np.testing.assert_array_equal(dwconv_ref.window_reverse(win, 2, res, res, ws, padded).reshape(-1, 3), win.reshape(-1, 3)[R.reverse_rows(2, res, res, ws)])
    for H, W in T.SWIN_MERGE_MAPS:  # the concat order of swin.cpp:150-154 in its usual spelling: x0 | x1 | x2 | x3 = [0::2, 0::2] | [1::2, 0::2] | [0::2, 1::2] | [1::2, 1::2]
        g = R.merge_gather(2, H, W).reshape(2, H // 2, W // 2, 4)
        oy, ox = np.meshgrid(np.arange(H // 2), np.arange(W // 2), indexing="ij")
        for part, (dy, dx) in enumerate(((0, 0), (1, 0), (0, 1), (1, 1))):
            for b in range(2):
                np.testing.assert_array_equal(g[b, :, :, part], (b * H + 2 * oy + dy) * W + 2 * ox + dx)


def test_depthwise_and_gelu_references_match_the_older_ones_and_the_oracle():
    for cid in ("dw-s1-5x17-c24", "dw-s2-5x9-c24", "dw-s2-2x2-c8", "dw-s1-1x1-c8", "dw-s2-b2-9x57-c160-blocks"):
        a = T.materialize(T.case(cid))
        x, w, b = R.f64(a["x"]), R.f64(a["w"]), R.f64(a["bias"])
        mine = R.depthwise3x3(x, w, a["stride"]) + b
        np.testing.assert_allclose(mine, dwconv_ref.depthwise_conv2d(x, w.reshape(3, 3, -1), b, a["stride"], 1), rtol=0, atol=1e-12)
        got = np.stack([oracle.conv2d_depthwise_nhwc(x[i], w.reshape(3, 3, -1), b, a["stride"], 1) for i in range(x.shape[0])])
        assert got.shape == mine.shape and np.abs(got - mine).max() < 17 * R.U32 * np.abs(mine).max() + 1e-7  # 9 products and a bias in f32
    v = np.linspace(-12, 12, 481)
    assert np.abs(oracle.gelu(v.astype(F32), oracle.GELU_TANH_F32) - R.gelu(v)).max() < 2e-6
    np.testing.assert_allclose(R.gelu(v), dwconv_ref.gelu_tanh(v), rtol=0, atol=1e-15)


def test_adds_are_exact_in_float64_and_their_f32_sum_rounds_once():
    """f16 + f16: exact in float64, and f16(f32(a + b)) = f16(a + b): the allowance-0 cases ask for bit equality"""
    rng = np.random.default_rng(2)
    a = rng.integers(0, 1 << 16, 200000).astype(np.uint16).view(np.float16)
    b = rng.integers(0, 1 << 16, 200000).astype(np.uint16).view(np.float16)
    ok = np.isfinite(a) & np.isfinite(b)
    a, b = a[ok], b[ok]
    with np.errstate(over="ignore"):
        np.testing.assert_array_equal((a.astype(F32) + b.astype(F32)).astype(np.float16).view(np.uint16), (a.astype(np.float64) + b.astype(np.float64)).astype(np.float16).view(np.uint16))
    c = T.materialize(T.case("addrows-inexact-f32"))
    s32 = c["a"] + c["b"].astype(F32)[np.arange(c["n"]) % c["period"]]
    assert (s32.astype(np.float64) != R.add_rows(c)[0]).mean() > 0.5  # the f32 sum is inexact in most elements


# ---- 2. the tables --------------------------------------------------------------------------------------------------------------------------------

def test_tables_span_what_the_issue_names():
    g = T.group
    assert {(c["C"], c["M"]) for c in g("ln32") if c["kind"] == "normal"} >= {(C, M) for C in (128, 384, 768, 1024, 1, 8, 63, 64, 65, 200, 1536) for M in (1, 4, 5, 131)}
    tv = g("tv_ln")
    assert {(c["C"], (c["res"], c["ws"]), c["out_f32"]) for c in tv} >= {(C, lay, o) for C in (8, 128, 136, 256, 264, 512, 520, 768, 1024) for lay in ((0, 0), (10, 4), (9, 4), (7, 7)) for o in (0, 1)}
    for C in T.TV_LN_C:  # rows that do not fill the last block, for every group width
        assert any(c["C"] == C and c["rows_out"] % R.tv_ln_rows_per_block(C) for c in tv)
    sw = g("swin_ln")
    assert {(c["C"], c["out_f32"]) for c in sw if not c["ws"]} == {(C, o) for C in (8, 128, 136, 256, 264, 512, 520, 1024, 1032, 2048) for o in (0, 1)}
    every = {((H, W), win) for H, W in ((9, 8), (5, 13), (7, 7), (14, 21)) for win in ((7, 0), (7, 3), (4, 1), (4, 3))}
    for C in T.SWIN_LN_C:
        of = {((c["H"], c["W"]), (c["ws"], c["shift"])) for c in sw if c["C"] == C and c["ws"]}
        assert {m for m, _ in of} == {m for m, _ in every} and (of >= every if C in (8, 136) else len(of) >= 4), C
    assert {((c["H"], c["W"]), (c["ws"], c["shift"])) for c in sw if c["ws"] and c["C"] not in (8, 136) and c["kind"] == "normal"} >= every
    assert all(c["B"] == 2 and not c["out_f32"] for c in sw if c["ws"])
    st = g("swin_ln_strided")
    assert {(c["C"], c["ldy"], c["out_f32"]) for c in st} >= {(C, ld, o) for C in T.SWIN_LN_C for ld in (C + 8, 2 * C) for o in (0, 1)}
    mg = g("swin_merge")
    assert {(c["C"], (c["H"], c["W"])) for c in mg} >= {(C, hw) for C in (8, 32, 40, 64, 72, 128, 136, 256, 264, 512, 520, 1024) for hw in ((2, 2), (4, 6), (6, 10))}
    assert all(c["B"] == 2 for c in mg)
    assert {(c["C"], (c["H"], c["W"]), (c["ws"], c["shift"])) for c in g("swin_reverse")} == {(C, m, w) for C in (8, 96) for m, w in every}
    assert {(c["C"], (c["res"], c["ws"])) for c in g("tv_reverse")} == {(C, lay) for C in (8, 96) for lay in ((10, 4), (9, 4), (7, 7))}
    dw = g("dwconv")
    for stride, widths in ((1, (1, 7, 8, 9, 17)), (2, (1, 2, 7, 8, 9))):
        assert {(c["W"], c["H"], c["C"], c["gelu"]) for c in dw if c["stride"] == stride and c["B"] == 2} >= {(W, H, C, ge) for W in widths for H in (1, 2, 5) for C in (8, 24, 160) for ge in (0, 1)}
    assert {(c["n"], c["b"]) for c in g("add_gelu")} >= {(n, b) for n in (8, 2056, 8000) for b in (0, 1)}
    ar = g("add_rows")
    for n in (8, 2056, 8000):
        for f32 in (0, 1):
            periods = {c["period"] for c in ar if c["n"] == n and c["a_is_f32"] == f32 and c["kind"] == "normal"}
            assert n in periods and any(n % p for p in periods) and (n == 8 or any(p < n and n % p == 0 for p in periods))
    assert {c["kind"] for c in g("dwconv")} == {"normal", "huge"} == {c["kind"] for c in g("add_gelu")} and {c["kind"] for c in ar} == {"normal", "inexact"}


def test_every_dispatch_class_is_hit_boundaries_included():
    assert {T.ln32_class(c["C"]) for c in T.group("ln32")} == T.LN32_CLASSES
    assert {T.tv_ln_class(c["C"]) for c in T.group("tv_ln")} - {(3, "mid")} == T.chain_classes(T.TV_LN_BOUNDS)  # (768 lies inside the wide class)
    for name in ("swin_ln", "swin_ln_strided"):
        assert {T.swin_ln_class(c["C"]) for c in T.group(name)} == T.chain_classes(T.SWIN_LN_BOUNDS)
    assert {T.swin_merge_class(c["C"]) for c in T.group("swin_merge")} == T.chain_classes(T.SWIN_MERGE_BOUNDS)
    # window mode and both output types in every class
    for name, klass in (("tv_ln", T.tv_ln_class), ("swin_ln", T.swin_ln_class)):
        for ws in (False, True):
            assert {klass(c["C"])[0] for c in T.group(name) if bool(c["ws"]) == ws} == set(range(len(T.TV_LN_BOUNDS if name == "tv_ln" else T.SWIN_LN_BOUNDS)))
    # every data kind at the smallest width of every class, for every LayerNorm entry point; eps both ways on the `tiny` rows; a zero bias each
    smallest = {"ln32": {128: "vec1", 384: "vec3", 768: "vec6", 1024: "vec8", 1: ("generic", "<64"), 64: ("generic", "=64"), 65: ("generic", ">64")},
                "tv_ln": {C: T.tv_ln_class(C) for C in (8, 136, 264, 520)}, "swin_ln": {C: T.swin_ln_class(C) for C in (8, 136, 264, 520, 1032)},
                "swin_ln_strided": {C: T.swin_ln_class(C) for C in (8, 136, 264, 520, 1032)}, "swin_merge": {C: T.swin_merge_class(C) for C in (8, 40, 72, 136, 264, 520)}}
    for name in LN_GROUPS:
        grp = T.group(name)
        for C, klass in smallest[name].items():
            assert klass == "vec" + str(C // 128) or klass[1] in ("lo", "<64", "=64", ">64"), (name, C)
            assert {c["kind"] for c in grp if c["C"] == C} == set(T.KINDS), (name, C)
            assert {c["eps"] for c in grp if c["C"] == C and c["kind"] == "tiny"} == {1e-5, 1e-6}, (name, C)
        assert {c["eps"] for c in grp} == {1e-5, 1e-6} and any(c.get("zero_bias") for c in grp)
        assert len({klass for klass in smallest[name].values() if isinstance(klass, str) or klass[1] != "mid"}) == len(smallest[name])
    for c in _ln_cases():
        a = T.materialize(c)
        assert (a["w"] == 0).any() or a["w"].size < 2
        assert (a["w"] < 0).any() or a["w"].size < 4
        assert bool(c.get("zero_bias")) == (not a["b"].any())
    # the depthwise block counts, from the launcher's own formula; and its block order is a permutation for each of them
    blocks = {T.dwconv_blocks(c) for c in T.group("dwconv")}
    assert blocks >= {1, 7, 8, 9} and any(b >= 17 and b % 8 for b in blocks), blocks
    for stride in (1, 2):
        assert {T.dwconv_blocks(c) for c in T.group("dwconv") if c["stride"] == stride} >= {1, 7, 9}
    for n in blocks:
        assert sorted(T.dwconv_block_order(n).tolist()) == list(range(n))
    assert sorted(T.dwconv_blocks(dict(B=b, H=h, W=w, C=ch, stride=s)) for s, b, h, w, ch in T.DW_BLOCK_SHAPES) == [7, 7, 8, 9, 9, 19]


def test_data_kinds_are_what_they_claim():
    rng = np.random.default_rng(5)
    x = T.rows_data("normal", 400, 256, rng)
    assert abs(x.mean() - 0.3) < 0.05 and abs(x.std() - 2) < 0.05
    x = T.rows_data("offset", 400, 256, rng)
    assert abs(x.mean() - 40) < 0.05 and abs(x.std() - 0.5) < 0.02
    x = T.rows_data("tiny", 400, 256, rng)
    assert abs(x.std() - 2e-3) < 1e-4 and x.var(axis=1).max() < 1e-5  # eps 1e-5 outweighs the variance, eps 1e-6 is a fifth of it
    x = T.rows_data("constant", 40, 24, rng)
    assert (np.ptp(x, axis=1) == 0).all() and len(set(x[:, 0].tolist())) == 40
    x = T.rows_data("outlier", 40, 24, rng)
    assert ((np.abs(x) == 60000).sum(axis=1) == 1).all() and {-60000.0, 60000.0} <= set(x.reshape(-1).tolist())
    x = T.rows_data("scales", 40, 2048, rng)
    sd = x.std(axis=1)
    assert np.allclose(sd[:17] / sd[0], 2.0 ** np.arange(17), rtol=0.1) and np.allclose(sd[17:34], sd[:17], rtol=0.1)
    for cid, key in (("dw-s1-5x9-c24-huge-gelu", "x"), ("dw-s2-5x9-c24-huge", "x"), ("addgelu-huge", "a"), ("addgelu-huge-nob", "a")):
        c = T.case(cid)
        a = T.materialize(c)
        s = (R.depthwise3x3(R.f64(a["x"]), R.f64(a["w"]), a["stride"]) + R.f64(a["bias"])) if c["entry"] == "dwconv" else R.f64(a["a"]) + (0 if a["b"] is None else R.f64(a["b"]))
        assert set(T.GELU_PLANTS) <= set(s.reshape(-1).tolist()) and np.abs(s).max() < 65504 and np.median(np.abs(s)) > 16384, cid


def test_the_canary_is_no_value_a_call_writes_and_the_guard_is_a_block():
    n = 0
    for c in T.all_cases():
        a = T.materialize(c)
        guard = T.guard_of(c, a)
        want, allow, written = R.evaluate(c["entry"], a, guard)
        assert np.isfinite(want).all() and np.isfinite(allow).all() and (allow >= 0).all()
        assert (np.abs(want - R.CANARY) > allow + 1000)[written].all(), c["id"]
        assert not written[-guard:].any() and (want[~written] == R.CANARY).all() and not allow[~written].any()
        assert written.sum() < 1.3e6 and guard >= R.min_guard(c["entry"], a) > 0  # small shapes; a block of rows behind the last one
        if c["entry"] == "swin_ln_strided" and a["ldy"] > a["C"]:
            assert (~written[:-guard]).sum() == (a["ldy"] - a["C"]) * a["rows_out"]  # the gap columns
        z = R.zero_bit_elements(c["entry"], a, want.size)
        assert z.any() == (c["entry"] == "swin_ln" and c["ws"] > 0 and (c["H"] % c["ws"] > 0 or c["W"] % c["ws"] > 0)) and not want[z].any() and written[z].all()
        n += 1
    assert n > 700


# ---- 3. a float32 emulation of the LayerNorm kernels, with the defects it can carry --------------------------------------------------------------

def _lane_layout(entry, width):
    """-> (lanes, slot of every channel in its lane, lane of every channel, slots per lane)"""
    c = np.arange(width)
    if entry == "ln32":
        if width in T.LN32_VECTOR:  # float2 vectors: pair p in lane p % 64
            return 64, (c // 2 // 64) * 2 + c % 2, (c // 2) % 64, width // 64
        return 64, c // 64, c % 64, -(-width // 64)
    if entry == "tv_ln":
        lanes, chunks = (16, 1) if width <= 128 else (32, 1) if width <= 256 else (64, 1) if width <= 512 else (64, 2)
    else:
        lanes, chunks = R.swin_ln_lanes(width)
    k = c // 8
    return lanes, (k // lanes) * 8 + c % 8, k % lanes, chunks * 8


def _row_sum(v, lanes, slot, lane, per, order, dead_value=None):
    """f32 sum of v [rows, width]: serial per lane, then an xor tree over the lanes; `order` 0 walks the slots upwards and the tree from the
    widest step, 1 the other way round. dead_value [rows, 1]: what the slots beyond the row's width hold (default 0)"""
    rows = v.shape[0]
    grid = np.zeros((rows, lanes, per), F32)
    if dead_value is not None:
        grid[:] = dead_value[:, :, None]
    grid[:, lane, slot] = v
    part = np.zeros((rows, lanes), F32)
    for s in (range(per) if order == 0 else range(per - 1, -1, -1)):
        part = part + grid[:, :, s]
    steps = [1 << i for i in range(lanes.bit_length() - 1)]
    for o in (steps[::-1] if order == 0 else steps):
        part = part + part[:, np.arange(lanes) ^ o]
    assert part.dtype == F32
    return part[:, :1]


def _window_src(Bn, H, W, ws, shift, defect=None):
    """the kernels' own index arithmetic, row by row (not the reference's pad / roll / reshape): window row -> source pixel or -1.
    `window_rows_cols_exchanged`: the window index is split by the number of window ROWS where the number of window columns belongs"""
    N, nwx, nwy = ws * ws, -(-W // ws), -(-H // ws)
    hp, wp = nwy * ws, nwx * ws
    row = np.arange(Bn * nwx * nwy * N)
    win, t = row // N, row % N
    iy, ix = t // ws, t % ws
    img, wi = win // (nwx * nwy), win % (nwx * nwy)
    per_row = nwy if defect == "window_rows_cols_exchanged" else nwx
    wy, wx = wi // per_row, wi % per_row
    s = -shift if defect == "shift_sign" else shift
    sy, sx = wy * ws + iy + s, wx * ws + ix + s
    sy, sx = np.where(sy >= hp, sy - hp, sy), np.where(sx >= wp, sx - wp, sx)
    sy, sx = np.where(sy < 0, sy + hp, sy), np.where(sx < 0, sx + wp, sx)
    return np.where((sy < H) & (sx < W), (img * H + sy) * W + sx, -1)


def _reverse_row(Bn, H, W, ws, shift, defect=None):
    """the kernels' own index arithmetic: pixel -> window row"""
    N, nwx, nwy = ws * ws, -(-W // ws), -(-H // ws)
    hp, wp = nwy * ws, nwx * ws
    pix = np.arange(Bn * H * W)
    img, t = pix // (H * W), pix % (H * W)
    s = -shift if defect == "shift_sign" else shift
    py, px = (t // W - s) % hp, (t % W - s) % wp
    per_row = nwy if defect == "window_rows_cols_exchanged" else nwx
    return np.minimum(((img * nwy + py // ws) * per_row + px // ws) * N + (py % ws) * ws + px % ws, Bn * nwx * nwy * N - 1)


def _source(entry, a, defect):
    """the rows as the kernel gathers them, with the gather defects -> (x f32 [rows, width], pad)"""
    C = a["C"]
    if entry == "swin_merge":
        g = R.merge_gather(a["B"], a["H"], a["W"])
        if defect == "merge_parts_by_row":
            g = g[:, [0, 2, 1, 3]]
        return R.f64(a["x"]).reshape(-1, C)[g].reshape(-1, 4 * C).astype(F32), np.zeros(g.shape[0], bool)
    if entry in ("tv_ln", "swin_ln") and a["ws"]:
        Bn, H, W, ws, shift = (a["B"], a["res"], a["res"], a["ws"], 0) if entry == "tv_ln" else (a["B"], a["H"], a["W"], a["ws"], a["shift"])
        src = _window_src(Bn, H, W, ws, shift, defect)
        x = R.f64(a["x"]).reshape(-1, C)
        return np.where((src < 0)[:, None], 0.0, x[np.maximum(src, 0)]).astype(F32), src < 0
    x, pad = R.layer_norm_source(entry, a)
    return x.astype(F32), pad


def emulate_ln(entry, a, guard, order=0, defect=None):
    """-> the whole output buffer as evaluate() lays it out, in the output type"""
    x, pad = _source(entry, a, defect)
    rows, width = x.shape
    lanes, slot, lane, per = _lane_layout(entry, width)
    swin = entry.startswith("swin")
    eps = a["eps"]
    if defect == "eps_dropped":
        eps = 0.0
    elif defect == "eps_other":
        eps = 1e-6 if eps == 1e-5 else 1e-5
    n = F32(lanes * per if defect == "mean_over_padded_width" else width)
    inv = F32(1) / n
    s = _row_sum(x, lanes, slot, lane, per, order)
    mean = s / n if swin else s * inv
    d = x - mean
    sq = (d.astype(np.float64) ** 2).astype(F32) if order == 0 else d * d
    q = _row_sum(sq, lanes, slot, lane, per, order, dead_value=(mean * mean) if defect == "dead_lanes_in_variance" else None)
    nv = F32(max(width - 1, 1) if defect == "variance_over_c_minus_1" else width)
    var = (q / nv + F32(eps)) if swin else (q.astype(np.float64) * np.float64(F32(1) / nv) + np.float64(F32(eps))).astype(F32)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        rstd = (1.0 / np.sqrt(var.astype(np.float64))).astype(F32)
        w, b = a["w"].astype(F32), a["b"].astype(F32)
        y = (d * rstd * w + b) if order == 0 else ((d * rstd).astype(np.float64) * w + b).astype(F32)  # separate roundings | the last two fused
    assert y.dtype == F32
    if pad.any():
        bias_rows = entry == "tv_ln"
        if defect == "pad_rows_normalised_not_zeroed" and swin:
            bias_rows = True
        if defect == "pad_rows_zeroed_not_bias" and entry == "tv_ln":
            bias_rows = False
        y[pad] = b if bias_rows else F32(0)
    dtype = R.out_dtype(entry, a)
    ld = (a.get("ldy") or width) if entry == "swin_ln_strided" else width
    buf = R.canary_buffer(rows * ld + guard, dtype)
    idx = np.arange(rows)[:, None] * ld + np.arange(width)[None, :]
    with np.errstate(over="ignore"):
        buf[idx] = y.astype(dtype)
        if defect == "last_row_into_guard":
            buf[idx[-1] + ld] = y[-1].astype(dtype)
            buf[idx[-1]] = R.CANARY
    return buf


def emulate_reverse(entry, a, guard, defect=None):
    C = a["C"]
    H, W, shift = (a["res"], a["res"], 0) if entry == "tv_reverse" else (a["H"], a["W"], a["shift"])
    ws, Bn = a["ws"], a["B"]
    rows = _reverse_row(Bn, H, W, ws, shift, defect)
    buf = R.canary_buffer(Bn * H * W * C + guard, np.float16)
    buf[:Bn * H * W * C] = (a["x"].astype(F32).reshape(-1, C) + a["a"].astype(F32).reshape(-1, C)[rows]).astype(np.float16).reshape(-1)
    return buf


def _reject(c, defect=None, order=0):
    """-> (the comparison's verdict on the emulation of case c, the violations)"""
    a = T.materialize(c)
    guard = T.guard_of(c, a)
    ref = R.evaluate(c["entry"], a, guard)
    got = emulate_ln(c["entry"], a, guard, order, defect) if c["entry"] in LN_GROUPS else emulate_reverse(c["entry"], a, guard, defect)
    v = violations(got, ref, untouched=R.CANARY)
    return rejected(v), v


def test_emulated_layer_norm_is_inside_the_allowance_for_every_case_in_two_orders():
    worst = defaultdict(float)
    for c in _ln_cases() + T.group("swin_reverse") + T.group("tv_reverse"):
        for order in (0, 1):
            bad, v = _reject(c, None, order)
            assert not bad, (c["id"], order, v)
            key = (c["entry"], c["kind"], "f32" if c.get("out_f32") else "f16")
            worst[key] = max(worst[key], v["ratio"])
    print("\nlargest emulated error / allowance per entry, data kind and output type:")
    for k, r in sorted(worst.items()):
        print(f"  {k[0]:16s} {k[1]:9s} {k[2]}  {r:.3f}")
    # no blanket: the f16 rounding alone brings the emulation close to it where v_rsq_f32's assumed figure does not dominate
    assert max(r for k, r in worst.items() if k[2] == "f16" and k[0] in LN_GROUPS) > 0.5
    assert all(r == 0 for k, r in worst.items() if k[0] in ("swin_reverse", "tv_reverse"))


def _small(c):
    return _width(c) <= 520 and c.get("rows_out", 0) <= 300


DEFECTS = {  # defect -> the cases it is tried on
    "variance_over_c_minus_1": lambda c: c["entry"] in LN_GROUPS and c["kind"] == "normal" and 1 < _width(c) <= 264 and not c.get("out_f32"),
    "eps_dropped": lambda c: c["entry"] in LN_GROUPS and c["kind"] in ("tiny", "constant") and _small(c),
    "eps_other": lambda c: c["entry"] in LN_GROUPS and c["kind"] == "tiny" and _small(c),
    "dead_lanes_in_variance": lambda c: c["entry"] in ("tv_ln", "swin_ln", "swin_ln_strided", "swin_merge") and c["kind"] in ("normal", "offset") and _small(c),
    "mean_over_padded_width": lambda c: c["entry"] in ("tv_ln", "swin_ln", "swin_ln_strided", "swin_merge") and c["kind"] in ("normal", "offset") and _small(c),
    "pad_rows_normalised_not_zeroed": lambda c: c["entry"] == "swin_ln" and c["ws"] and (c["H"] % c["ws"] or c["W"] % c["ws"]) and not c.get("zero_bias") and _small(c),
    "pad_rows_zeroed_not_bias": lambda c: c["entry"] == "tv_ln" and c["ws"] and c["res"] % c["ws"] and not c.get("zero_bias") and _small(c),
    "shift_sign": lambda c: c["entry"] in ("swin_ln", "swin_reverse") and c.get("shift") and _small(c),
    "window_rows_cols_exchanged": lambda c: c["entry"] in ("swin_ln", "swin_reverse") and c.get("ws") and _small(c),
    "merge_parts_by_row": lambda c: c["entry"] == "swin_merge" and c["kind"] == "normal" and _small(c),
    "last_row_into_guard": lambda c: c["entry"] in LN_GROUPS and c["kind"] == "normal" and _small(c),
}


def test_seeded_defects_are_rejected_by_the_comparison_the_gpu_test_uses():
    print()
    for defect, applies in DEFECTS.items():
        tried = [c for c in T.all_cases() if applies(c)]
        rejecting = [c for c in tried if _reject(c, defect)[0]]
        print(f"{defect}: rejected by {len(rejecting)} of the {len(tried)} cases tried: " + ", ".join(c["id"] for c in rejecting[:6]) + (" ..." if len(rejecting) > 6 else ""))
        missed = [c["id"] for c in tried if c not in rejecting]
        if missed:
            print("    not rejected by: " + ", ".join(missed[:12]) + (" ..." if len(missed) > 12 else ""))
        assert rejecting, defect
        by_entry = {c["entry"] for c in rejecting}
        assert by_entry == {c["entry"] for c in tried}, (defect, by_entry)  # every entry point the defect can live in rejects it
        if defect == "variance_over_c_minus_1":  # above 264 it sinks below RSQ_REL plus the f16 rounding: a limit of the assumed constant, stated in DESIGN.md
            assert not missed, missed
            wider = [c for c in _ln_cases() if c["kind"] == "normal" and 264 < _width(c) <= 1032 and not c.get("out_f32") and c.get("rows_out", 0) <= 300]
            seen = defaultdict(lambda: [0, 0])
            for c in wider:
                seen[(c["entry"], _width(c))][0] += _reject(c, defect)[0]
                seen[(c["entry"], _width(c))][1] += 1
            print("    beyond the widths it must show at (reported, not asserted), rejected / tried: " + ", ".join(f"{e} {w}: {r}/{n}" for (e, w), (r, n) in sorted(seen.items())))
        if defect == "window_rows_cols_exchanged":  # a square window grid cannot show it
            for c in tried:
                square = -(-c["H"] // c["ws"]) == -(-c["W"] // c["ws"])
                assert (c in rejecting) == (not square), c["id"]
        if defect in ("dead_lanes_in_variance", "mean_over_padded_width"):  # every width that leaves a chunk dead shows it, no other can
            for c in tried:
                lanes, _, _, per = _lane_layout(c["entry"], _width(c))
                assert (c in rejecting) == (lanes * per > _width(c)), c["id"]
        if defect in ("eps_dropped", "eps_other"):
            assert {c["id"] for c in tried if c["kind"] == "tiny" and _width(c) > 1} <= {c["id"] for c in rejecting}  # (a row of one element is its own mean)
        if defect == "last_row_into_guard":  # under its own keys: a row of stray stores in the guard; outside are those and the row left at the canary
            for c in tried:
                v = _reject(c, defect)[1]
                assert v["stray"] == _width(c) and v["outside"] == 2 * _width(c) and v["first_stray"] >= v["ratios"].size - T.guard_of(c, T.materialize(c)) and v["nonfinite"] == 0, c["id"]
        if defect == "eps_dropped":  # a constant row without eps is 0 x inf
            for c in tried:
                if c["kind"] == "constant":
                    v = _reject(c, defect)[1]
                    assert v["nonfinite"] > 0 and v["stray"] == 0 and v["ratio"] == np.inf, c["id"]
        if defect in ("shift_sign", "merge_parts_by_row", "last_row_into_guard", "pad_rows_zeroed_not_bias", "pad_rows_normalised_not_zeroed"):  # (a zero bias cannot tell the pad rows' two contents apart)
            assert not missed, missed


# ---- 4. the refusals ----------------------------------------------------------------------------------------------------------------------------

def test_refusal_tables_return_before_any_launch():
    """host code: every refusal is decided before the first HIP call, so the tables run without a device (the operands are one host buffer)"""
    names = {"C not a multiple of 8": [("tv_ln", dict(C=12)), ("swin_ln", dict(C=12)), ("swin_merge", dict(C=12)), ("dwconv", dict(C=12)), ("swin_reverse", dict(C=12)), ("tv_reverse", dict(C=12))],
             "C above each limit": [("tv_ln", dict(C=1032)), ("swin_ln", dict(C=2056)), ("swin_merge", dict(C=1032))],
             "rows that do not form whole images": [("tv_ln", dict(res=10, ws=4, rows_out=100)), ("swin_ln", dict(rows_out=60))],
             "shift >= ws": [("swin_ln", dict(shift=4)), ("swin_reverse", dict(shift=4))], "window mode with f32 output": [("swin_ln", dict(out_f32=1))],
             "an odd map": [("swin_merge", dict(H=3)), ("swin_merge", dict(W=5))], "ldy": [("swin_ln_strided", dict(ldy=56)), ("swin_ln_strided", dict(ldy=68))],
             "stride 3": [("dwconv", dict(stride=3))], "n or the period": [("add_gelu", dict(n=12)), ("add_rows", dict(n=12)), ("add_rows", dict(period=12))],
             "the three launcher checks": [("ln32", dict(x=0)), ("ln32", dict(w=0)), ("ln32", dict(b=0)), ("ln32", dict(y=0)), ("dwconv", dict(C=0)), ("tv_reverse", dict(C=0))]}
    for what, entries in names.items():
        for entry, fields in entries:
            assert any(f == fields for f, _ in T.REFUSAL_TABLES[entry]), (what, entry, fields)
    assert T.N_REFUSALS > 90
    src = {n: (Path(__file__).resolve().parents[1] / "vision.cpp_amd" / "csrc" / n).read_text() for n in ("kernels_misc.hip", "kernels_tinyvit.hip")}
    assert re.search(r"vx_layernorm_f32_f16\([^{]*\{\s*VX_REQUIRE\(x && w && b && y,", src["kernels_misc.hip"])
    assert "C > 0 && C % 8 == 0 && (stride == 1 || stride == 2)" in src["kernels_tinyvit.hip"] and 'ws > 0 && C > 0 && C % 8 == 0, "vx_window_reverse_add_f16' in src["kernels_tinyvit.hip"]
    if L.get_lib().vx_device_count() > 0:
        return  # with a device the GPU suite runs the tables, on device memory (a refusal that regressed would launch on these host operands)
    scratch = np.zeros(T.REFUSAL_SCRATCH_BYTES, np.uint8)
    seen = []
    assert T.run_refusals(L.get_lib(), scratch.ctypes.data, seen) == T.N_REFUSALS
    assert not scratch.any() and len(seen) == T.N_REFUSALS

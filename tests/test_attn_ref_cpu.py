"""No device: the float64 references of the attention kernels (tests/attn_ref.py) are pinned to the CPU oracle, graph_window_ref and cross_attn_ref, numpy
emulations of each kernel's arithmetic (f16 P, the packed-f16 add tree, f32 sums, the lagging reference point) lie inside the allowance on every
case of tests/attn_cases.py, seeded corruptions of those emulations lie outside, every key of every case is visible through the allowance, the
case table reaches what the launchers can select, and the two host packers lay the bias out in accumulator order."""
import functools

import numpy as np
import pytest

import attn_cases as T
import attn_ref as R
import cross_attn_ref as XR
import graph_window_ref as GW
from buffer_check import rejected, violations
from oracle import oracle as O
from visioncpp_amd import _lib as L

LOG2E = np.float32(R.LOG2E)


@functools.lru_cache(maxsize=None)
def _made(case_id):
    case = next(c for c in T.ALL if c["id"] == case_id)
    a = T.materialize(case)
    return a, R.evaluate(a["entry"], a)


def _ids(cases):
    return [c["id"] for c in cases]


# ---- 1. the references against the oracle and graph_window_ref ------------------------------------------------------------------------------

@pytest.mark.parametrize("case_id", ["T65-B2-H8", "T257-B1-H3", "low-T200"])
def test_attention_reference_matches_the_cpu_oracle(case_id):
    a, (want, allow, written) = _made(case_id)
    B, H, Tn = a["B"], a["H"], a["T"]
    tok = lambda x: np.ascontiguousarray(x.astype(np.float32).transpose(0, 2, 1, 3).reshape(B, Tn, H * 64))  # noqa: E731
    q, k, v = tok(a["q"]), tok(a["k"]), tok(a["v"])
    got = np.concatenate([O.attention(q[b], k[b], v[b], H, 1.0 / R.LOG2E) for b in range(B)])   # q carries scale * log2(e): softmax(q k^T / log2e)
    # the oracle is f32: scores within (64 + 8) u32 sum|q||k| (<= 64 max|q| max|k|), sums of T terms; far below the f16 allowance
    bound = 2 * ((64 + 8) * R.U32 * 64 * np.abs(q).max() * np.abs(k).max() + (Tn + 8) * R.U32) * 2 * np.abs(v).max()
    assert np.abs(got - want).max() <= bound
    assert written.all() and (allow > 0).all()


@pytest.mark.parametrize("case_id", ["hd64-T49-f32-B4-Bm2-H3-Hm3-swin", "hd64-T96-f16-B2-Bm2-H2-Hm2-band-x", "hd32-T33-f16-B4-Bm2-H3-Hm1-standin"])
def test_masked_reference_matches_graph_window_ref(case_id):
    a, (want, _, _) = _made(case_id)
    tok = lambda x: x.astype(np.float64).transpose(0, 2, 1, 3)  # noqa: E731
    ref = GW.attention_masked(tok(a["q"]), tok(a["k"]), tok(a["v"]), a["mask"].astype(np.float64), 1.0 / R.LOG2E)
    assert np.abs(ref.reshape(want.shape) - want).max() <= 1e-12 * max(1.0, np.abs(want).max())


@pytest.mark.parametrize("case_id", ["N49-h1-w5", "ws8-3x1-h3", "ws7-2x3-h3"])
def test_window_reference_matches_graph_window_ref(case_id):
    a, (want, _, _) = _made(case_id)
    n_win, N, heads = a["n_windows"], a["N"], a["heads"]
    qkv = a["qkv"].astype(np.float64).reshape(n_win, N, heads, 3, 32)
    mask = a["bias"][None].astype(np.float64) + (0.0 if a["mask"] is None else a["mask"][:, None].astype(np.float64))
    ref = GW.attention_masked(qkv[..., 0, :], qkv[..., 1, :], qkv[..., 2, :], mask, 1.0 / np.sqrt(32.0))
    assert np.abs(ref.reshape(want.shape) - want).max() <= 1e-12 * max(1.0, np.abs(want).max())


@pytest.mark.parametrize("case", T.group("cross"), ids=_ids(T.group("cross")))
def test_cross_reference_matches_the_independent_statement(case):
    """cross_attn_ref.attention: natural exponent, einsum over all heads at once; evaluate_cross: exp2, per (b, h) problem. Both float64."""
    a, (want, allow, written) = _made(case["id"])
    ref = XR.attention(a["q"], a["k"], a["v"], float(np.float32(a["scale"]))).reshape(want.shape)
    # the scores differ by a few float64 roundings of a value of at most max|s| (natural log), which moves a weight by that relative amount
    smax = abs(a["scale"]) * np.einsum("bqhd,bkhd->bhqk", np.abs(a["q"].astype(np.float64)), np.abs(a["k"].astype(np.float64))).max()
    assert np.abs(ref - want).max() <= 2.0 ** -52 * (16 + 8 * smax + a["Tk"]) * np.abs(a["v"].astype(np.float64)).max()
    assert written.all() and (allow > 0).all()


def test_small_reference_matches_the_cpu_oracle():
    rng = np.random.default_rng(1)
    for hd, heads in ((4, 3), (32, 1)):
        q, k, v = (rng.standard_normal((33, heads * hd)).astype(np.float16) for _ in range(3))
        want = R.evaluate_small(dict(q=q, k=k, v=v, Nq=33, Nk=33, heads=heads, hd=hd))[0]
        got = O.attention(q.astype(np.float32), k.astype(np.float32), v.astype(np.float32), heads, 1.0 / np.sqrt(hd))
        assert np.abs(got - want).max() <= 2 * (hd + 33 + 16) * R.U32 * (1 + np.abs(q.astype(np.float64)).max() * np.abs(k.astype(np.float64)).max() * hd) * 4


# ---- 2. / 3. numpy emulations of the kernels' arithmetic, and corruptions of them -------------------------------------------------------------

def f32(x):
    return np.asarray(x, np.float32)


def r16(x):
    with np.errstate(over="ignore"):
        return f32(x).astype(np.float16).astype(np.float32)


def _tree_sum(P):
    """vx_attention_f16's tile row sum (VISP_ATTN_RS = 1): per lane half 16 packed pairs, four levels of f16 adds, the rest in f32. P: [Tq, 64]."""
    n = P.shape[0]
    x = P.reshape(n, 8, 2, 4).transpose(0, 2, 1, 3).reshape(n, 2, 16, 2)   # keys with (key & 4) set belong to the upper lane half
    with np.errstate(invalid="ignore"):
        for w in (8, 4, 2, 1):
            x = r16(x[:, :, :w] + x[:, :, w:2 * w])
        return f32(f32(x[:, 0, 0, 0] + x[:, 0, 0, 1]) + f32(x[:, 1, 0, 0] + x[:, 1, 0, 1]))


def _exp2(x):
    with np.errstate(over="ignore", invalid="ignore"):
        return np.exp2(f32(x)).astype(np.float32)


def _fma(a, b, c):
    """f32 fma: the product of two f32 is exact in float64, the sum rounds once there and once to f32"""
    return f32(np.float64(a) * np.float64(b) + np.float64(c))


def _emulate_cross(p, corrupt):
    """attention_cross_kernel and attention_cross_combine_kernel: f32 scores times the f32 qs, tail keys -inf, 32-key tiles, running maximum with floor
    -1e30, unrounded p into l, f16 P into the PV product, queries beyond T_q on the clamped row; a split leaves (m, l, O) per 128-key part and the
    combine folds them as written: m = max m_i, l and acc as fma chains in part order, acc * (1 / l)."""
    q, k, v = f32(p["q"]), f32(p["k"]), f32(p["v"])
    Tq, Tk, parts = q.shape[0], k.shape[0], p["parts"]
    qs = f32(p["qs"] / LOG2E) if corrupt == "scale_log2e" else p["qs"]
    s = f32(f32(q @ k.T) * qs)
    if corrupt == "drop_key":
        s[:, Tk // 2] = -np.inf
    if corrupt == "double_key":
        s[:, Tk // 2] += 1.0
    s = np.concatenate([s, np.repeat(s[-1:], -Tq % 32, 0)])
    n = s.shape[0]
    gain = np.float32(1.02 if corrupt == "p_bias" else 1.0)
    triples = []
    for part in range(parts):
        k0, k1 = (part * 128, min(Tk, part * 128 + 128)) if parts > 1 else (0, Tk)
        sp, vp = s[:, k0:k1], v[k0:k1]
        pad, fill = -(k1 - k0) % 32, -np.inf
        if part == parts - 1 and corrupt == "tail_unmasked":
            fill = 0.0
        if part == parts - 1 and corrupt == "part_tail":   # the part runs to k_begin + 128: its zero-staged keys score 0
            pad, fill = k0 + 128 - k1, 0.0
        sp, vp = np.pad(sp, ((0, 0), (0, pad)), constant_values=fill), np.pad(vp, ((0, pad), (0, 0)))
        o, l, m = np.zeros((n, vp.shape[1]), np.float32), np.zeros(n, np.float32), np.full(n, -1e30, np.float32)
        for t in range(sp.shape[1] // 32):
            st, vt = sp[:, t * 32:(t + 1) * 32], vp[t * 32:(t + 1) * 32]
            m_new = np.maximum(m, st.max(1))
            alpha = _exp2(m - m_new)
            l, o, m = f32(l * alpha), f32(o * alpha[:, None]), m_new
            pr = _exp2(st - m[:, None])
            l = f32(l + pr.sum(1, dtype=np.float32))
            o = f32(o + f32(r16(pr) * gain) @ vt)
        triples.append((m, l, o))
    if parts == 1:
        m, l, o = triples[0]
        return r16(o * f32(1.0 / l)[:, None])[:Tq].astype(np.float64)
    used = triples[:-1] if corrupt == "drop_part" else triples
    m = np.full(n, -1e30, np.float32)
    for mi, _, _ in used:
        m = np.maximum(m, mi)
    if corrupt == "stale_max":
        m = triples[0][0]
    l, acc = np.zeros(n, np.float32), np.zeros((n, v.shape[1]), np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        for mi, li, oi in used:
            w = _exp2(mi - m)
            l, acc = _fma(li, w, l), _fma(oi, w[:, None], acc)
        return r16(acc * f32(1.0 / l)[:, None])[:Tq].astype(np.float64)


def emulate(p, corrupt=None, limit=1024.0):
    """One problem of attn_ref.PROBLEMS on the kernel's own arithmetic -> the f16 output [Tq, hd] as float64. `corrupt` plants one defect."""
    if p["kind"] == "cross":
        return _emulate_cross(p, corrupt)
    q, k, v = f32(p["q"]), f32(p["k"]), f32(p["v"])
    Tq, Tk, kind = q.shape[0], k.shape[0], p["kind"]
    add = None if p["add"] is None else f32(p["add"])
    if corrupt == "neighbour_mask_row" and add is not None:
        add = np.roll(add, -1, axis=0)
    acc = q @ k.T
    if corrupt == "scale_log2e":
        acc = f32(acc / LOG2E)
    if kind == "small":
        s = f32(f32(q * np.float32(1.0 / np.sqrt(q.shape[1]))) @ k.T)
        if corrupt == "scale_log2e":
            s = f32(s / LOG2E)
        if corrupt == "drop_key":
            s[:, Tk // 2] = -np.inf
        pr = np.exp(f32(s - s.max(1, keepdims=True))).astype(np.float32)
        if corrupt == "double_key":
            pr[:, Tk // 2] *= 2
        out = (pr @ v) * f32(1.0 / pr.sum(1, dtype=np.float32))[:, None]
        return r16(out).astype(np.float64)
    if kind == "dense":
        s = acc
    elif kind == "masked":
        s = f32(add * LOG2E + acc)
    else:
        s = f32(f32(acc * np.float32(1.0 / np.sqrt(32.0)) + add) * LOG2E)
    if corrupt == "drop_key":
        s[:, Tk // 2] = -np.inf
    if corrupt == "double_key":
        s[:, Tk // 2] += 1.0
    tile = p["tile"]
    qpad, kpad = -Tq % 32, -Tk % tile
    s = np.pad(s, ((0, 0), (0, kpad)), constant_values=0.0 if corrupt == "tail_unmasked" else -np.inf)
    s = np.concatenate([s, np.repeat(s[-1:], qpad, 0)])   # queries beyond T are computed on the clamped row
    v = np.pad(v, ((0, kpad), (0, 0)))
    n = s.shape[0]
    o, l = np.zeros((n, v.shape[1]), np.float32), np.zeros(n, np.float32)
    m = np.zeros(n, np.float32) if kind == "dense" else np.full(n, -1e30, np.float32)
    gain = np.float32(1.02 if corrupt == "p_bias" else 1.0)
    for t in range(s.shape[1] // tile):
        st, vt = s[:, t * tile:(t + 1) * tile], v[t * tile:(t + 1) * tile]
        if kind == "dense":
            last = (t + 1) * tile > Tk
            full = np.ones(n, bool)
            P = psum = None
            if t > 0 and not last:
                P = r16(_exp2(st - m[:, None]))
                psum = _tree_sum(P)
                full = np.repeat(~(psum <= limit).reshape(-1, 32).all(1), 32)   # wave-uniform: 32 queries fall back together
            if full.any():
                with np.errstate(invalid="ignore"):
                    mloc = f32(st - m[:, None]).max(1)
                delta = mloc if t == 0 else np.maximum(mloc, np.float32(0))
                upd = full & (np.repeat((delta > 0).reshape(-1, 32).any(1), 32) | (t == 0))
                alpha = np.where(upd & (t > 0), _exp2(-delta), np.float32(1))
                l, o = f32(l * alpha), f32(o * alpha[:, None])
                m = np.where(upd, f32(m + delta), m)
                P2 = r16(_exp2(st - m[:, None]))
                P = P2 if P is None else np.where(full[:, None], P2, P)
                psum = _tree_sum(P2) if psum is None else np.where(full, _tree_sum(P2), psum)
            l = f32(l + psum)
            o = f32(o + f32(P * gain) @ vt)
        else:
            m_new = np.maximum(m, st.max(1))
            alpha = _exp2(m - m_new)
            l, o, m = f32(l * alpha), f32(o * alpha[:, None]), m_new
            pr = _exp2(st - m[:, None])
            l = f32(l + pr.sum(1, dtype=np.float32))
            o = f32(o + f32(r16(pr) * gain) @ vt)
    return r16(o * f32(1.0 / l)[:, None])[:Tq].astype(np.float64)


ARG_CORRUPTIONS = {   # defects that pick the wrong operand slice: applied to the arguments
    "mask_head": lambda a: dict(a, mask=np.roll(a["mask"], -1, axis=1)) if a["entry"] == "masked" and a["Hm"] > 1 else None,
    "mask_batch": lambda a: dict(a, mask=np.roll(a["mask"], -1, axis=0)) if a["entry"] == "masked" and a["Bm"] > 1 else None,
    "wrong_class": lambda a: dict(a, mask=np.roll(a["mask"], -1, axis=0)) if a["entry"] == "window" and a["nwx"] * a["nwy"] > 1 else None,
    "kv_head": lambda a: dict(a, k=np.roll(a["k"], -1, axis=2), v=np.roll(a["v"], -1, axis=2)) if a["entry"] == "cross" and a["H"] > 1 else None,
    "kv_batch": lambda a: dict(a, k=np.roll(a["k"], -1, axis=0), v=np.roll(a["v"], -1, axis=0)) if a["entry"] == "cross" and a["B"] > 1 else None,
}


def emulate_call(a, corrupt=None, limit=1024.0):
    """-> the whole output buffer of the call (no guard rows) as the emulation leaves a zeroed one"""
    if corrupt in ARG_CORRUPTIONS:
        a = ARG_CORRUPTIONS[corrupt](a)
        if a is None:
            return None
    rows, cols = R.out_shape(a["entry"], a)
    out = np.zeros((rows, cols))
    for p in R.PROBLEMS[a["entry"]](a):
        res = emulate(p, corrupt, limit)
        if corrupt == "block_shift":   # the output of query block i lands in the slot of block i + 1
            res = np.concatenate([np.zeros_like(res[:32]), res[:-32]])[:res.shape[0]]
        out[p["rows"], p["cols"]] = res
    return out


@pytest.mark.parametrize("case", T.ALL, ids=_ids(T.ALL))
def test_emulated_kernel_is_inside_the_allowance(case):
    a, ref = _made(case["id"])
    limits = (1024.0, 0.0) if case["entry"] == "attention" and case["T"] > 128 else (1024.0,)
    for limit in limits:
        v = violations(emulate_call(a, limit=limit), ref)  # the GPU test's comparison
        print(f"limit {limit}: emulation's largest err / allowance {v['ratio']:.3f}")
        assert not rejected(v), (limit, v["stray"], v["nonfinite"], v["outside"], v["ratio"])


# corruption -> {family: candidate cases}; every (corruption, family) pair must leave the allowance on at least one of them
def _pick(group, pred=lambda c: True, n=6):
    return [c for c in T.group(group) if pred(c)][:n]


_multi_q = lambda c: c.get("T", c.get("N", 0)) > 64  # noqa: E731
_split = lambda c: T.cross_parts(c["Tq"], c["Tk"]) > 1  # noqa: E731
CORRUPTIONS = {
    "drop_key": dict(attention=_pick("attention", lambda c: c["T"] > 1), masked=_pick("masked", lambda c: c["T"] > 1), window=_pick("window", lambda c: c["N"] > 1),
                     shifted=_pick("shifted"), small=_pick("small", lambda c: c["Nk"] > 1 and c["Nq"] >= c["Nk"]),
                     cross=_pick("cross", lambda c: c["Tk"] > 1 and c["Tq"] >= c["Tk"])),
    "double_key": dict(attention=_pick("attention", lambda c: c["T"] > 1), masked=_pick("masked", lambda c: c["T"] > 1), window=_pick("window", lambda c: c["N"] > 1),
                       shifted=_pick("shifted"), small=_pick("small", lambda c: c["Nk"] > 1 and c["Nq"] >= c["Nk"]),
                       cross=_pick("cross", lambda c: c["Tk"] > 1 and c["Tq"] >= c["Tk"])),
    "tail_unmasked": dict(attention=_pick("attention", lambda c: c["T"] % 64), masked=_pick("masked", lambda c: c["T"] % 32), window=_pick("window", lambda c: c["N"] % 32),
                          shifted=_pick("shifted", lambda c: c["N"] % 32), cross=_pick("cross", lambda c: c["Tk"] % 32)),
    "neighbour_mask_row": dict(masked=_pick("masked", lambda c: c["T"] > 1), window=_pick("window", lambda c: c["N"] > 1), shifted=_pick("shifted")),
    "mask_head": dict(masked=_pick("masked", lambda c: c["Hm"] > 1)),
    "mask_batch": dict(masked=_pick("masked", lambda c: c["Bm"] > 1)),
    "wrong_class": dict(shifted=_pick("shifted", lambda c: c["nwx"] * c["nwy"] > 1)),
    "scale_log2e": dict(attention=_pick("attention", lambda c: c["T"] > 1), masked=_pick("masked", lambda c: c["T"] > 1), window=_pick("window", lambda c: c["N"] > 1),
                        shifted=_pick("shifted"), small=_pick("small", lambda c: c["Nk"] > 1), cross=_pick("cross", lambda c: c["Tk"] > 1)),
    "p_bias": dict(attention=_pick("attention"), masked=_pick("masked"), window=_pick("window"), shifted=_pick("shifted"), cross=_pick("cross")),
    "block_shift": dict(attention=_pick("attention", _multi_q), masked=_pick("masked", _multi_q), window=_pick("window", _multi_q), shifted=_pick("shifted", _multi_q),
                        cross=_pick("cross", lambda c: c["Tq"] > 64)),
    # the key split of vx_attention_cross_f16: the combine skips the last part; the last part runs to k_begin + 128 and its zero-staged keys score 0 instead
    # of -inf; the combine takes part 0's maximum as the reference point (the same value as long as no weight overflows: the "cliff" data is what sees it)
    "drop_part": dict(cross=_pick("cross", _split)),
    "part_tail": dict(cross=_pick("cross", lambda c: _split(c) and c["Tk"] % 128)),
    "stale_max": dict(cross=_pick("cross", lambda c: _split(c) and c["data"] in ("spike", "ramp", "cliff"))),
    "kv_head": dict(cross=_pick("cross", lambda c: c["Tk"] > 1)),
    "kv_batch": dict(cross=_pick("cross", lambda c: c["Tk"] > 1 and c["B"] > 1)),
}
PAIRS = [(name, fam) for name, fams in CORRUPTIONS.items() for fam in fams]


@pytest.mark.parametrize("name,family", PAIRS, ids=[f"{n}-{f}" for n, f in PAIRS])
def test_seeded_corruption_leaves_the_allowance(name, family):
    cases = CORRUPTIONS[name][family]
    assert cases
    caught = []
    for case in cases:
        a, ref = _made(case["id"])
        got = emulate_call(a, name)
        assert got is not None, case["id"]
        if rejected(violations(got, ref)):   # the device comparison itself: a NaN is outside too
            caught.append(case["id"])
    assert caught, f"{name} stays inside the allowance on every one of {_ids(cases)}"


# ---- 4. every key is visible through the allowance ------------------------------------------------------------------------------------------------

SENSITIVITY = 4.0
WORST = {}


def _sensitive(c):
    """Dropping key j changes row i by p_ij (v_j - out_i) / (1 - p_ij). For the three MFMA kernels every case takes part (a lone key cannot be dropped).
    vx_small_attention_f16 takes part where Nq >= Nk: a query has at most 1 / p keys of weight p, so with fewer queries than keys most keys weigh
    less on every output than one f16 rounding of it, whatever the data.
    vx_attention_cross_f16 takes part with every key where Tq >= Tk. Where Tq < Tk the same counting holds, so the condition is asked of the keys of
    attn_cases.cross_edge_keys only (the first and last key of every 32-key block and 128-key part, and the last key: where a defect of the key loop can
    sit), each taken at the (b, h) problem that sees it best: the case's queries own those keys in turn over its problems, and a defect at a key position
    is the same in every problem. The data kinds built to be peaked ("spike", "ramp", "cliff") hide most keys on purpose and are exempt."""
    if c["entry"] == "small":
        return c["Nk"] > 1 and c["Nq"] >= c["Nk"]
    if c["entry"] == "cross":
        return c["Tk"] > 1 and c["data"] not in ("spike", "ramp", "cliff")
    return c.get("T", c.get("N")) > 1


@pytest.mark.parametrize("case", [c for c in T.ALL if _sensitive(c)], ids=_ids([c for c in T.ALL if _sensitive(c)]))
def test_dropping_any_key_moves_some_output_by_four_allowances(case):
    a, (want, allow, _) = _made(case["id"])
    worst, per_key = np.inf, None
    for p in R.PROBLEMS[a["entry"]](a):
        out, _, w = R.solve(p)
        al = allow[p["rows"], p["cols"]]
        with np.errstate(divide="ignore", invalid="ignore"):
            g = np.where(1.0 - w > 1e-9, w / (1.0 - w), 0.0)            # [Tq, Tk]; the only live key of a query cannot be dropped
        ratio = np.zeros(w.shape[1])
        for d in range(out.shape[1]):
            ratio = np.maximum(ratio, (g * np.abs(p["v"][None, :, d] - out[:, d, None]) / al[:, d, None]).max(0))
        worst = min(worst, float(ratio.min()))
        per_key = ratio if per_key is None else np.maximum(per_key, ratio)
    if case["entry"] == "cross":   # per key position, the problem that sees it best; with fewer queries than keys the edge keys only: _sensitive
        keys = slice(None) if case["Tq"] >= case["Tk"] else T.cross_edge_keys(case["Tq"], case["Tk"])
        worst = float(per_key[keys].min())
    WORST[case["id"]] = worst
    print(f"smallest key-sensitivity ratio {worst:.2f}")
    assert worst >= SENSITIVITY, worst


def test_report_the_smallest_sensitivity():
    if WORST:
        cid = min(WORST, key=WORST.get)
        print(f"smallest key-sensitivity ratio over {len(WORST)} cases: {WORST[cid]:.2f} ({cid})")


# ---- 5. the case table ------------------------------------------------------------------------------------------------------------------------------

def test_table_reaches_what_the_launchers_select():
    ids = _ids(T.ALL)
    assert len(set(ids)) == len(ids)
    # vx_attention_f16: both block shapes run every case through the hook; the default rule alone also picks both, and every listed grid occurs
    assert {T.attention_default_waves(c["T"]) for c in T.ATTENTION} == {4, 8}
    grids = {T.attention_grid(c, w) for c in T.ATTENTION for w in (4, 8)}
    assert set(T.GRID_SIZES) <= grids, sorted(set(T.GRID_SIZES) - grids)
    remap = {(g >> 3 > 0, g & 7 > 0) for g in grids}
    assert (True, True) in remap and (True, False) in remap and (False, True) in remap     # per > 0 with rem != 0, rem == 0, per == 0
    assert {c["T"] for c in T.ATTENTION} >= {1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 769, 1370}
    assert any(c["T"] == 513 and c["B"] > 1 and c["H"] > 1 for c in T.ATTENTION)
    # vx_attention_masked_f16: six instances, the idle-wave form (three query blocks on four waves), three blocks per head, both mask paths and types
    inst = {(c["head_dim"], T.masked_waves(c["T"])) for c in T.MASKED}
    assert inst == {(hd, nw) for hd in (32, 64) for nw in (1, 2, 4)}
    for hd in (32, 64):
        mine = [c for c in T.MASKED if c["head_dim"] == hd]
        assert {c["T"] for c in mine} == set(T.MASKED_T)
        assert any(64 < c["T"] <= 96 for c in mine) and any(-(-c["T"] // 128) >= 3 for c in mine)
        assert {(c["T"] % 4 == 0, c["mask_is_f32"]) for c in mine} == {(v, f) for v in (True, False) for f in (0, 1)}
        assert {c["content"] for c in mine} == {"random", "band", "standin", "swin"}
        assert {c["Hm"] == 1 for c in mine} == {True, False} and {c["Bm"] for c in mine} >= {1, 2, 3}
        assert all(c["H"] > 1 for c in mine)
    # window kernels: every block shape, plain and with class masks
    assert {T.window_qb(c["N"]) for c in T.WINDOW} == {1, 2, 4, 7, 8} == {T.window_qb(c["N"]) for c in T.SHIFTED}
    assert {c["N"] for c in T.WINDOW} == set(T.WINDOW_N) and {c["ws"] for c in T.SHIFTED} == set(T.SHIFT_WS)
    assert {(c["nwx"], c["nwy"]) for c in T.SHIFTED} == {(1, 1), (3, 1), (2, 3)} and {c["heads"] for c in T.WINDOW} == {1, 3} == {c["heads"] for c in T.SHIFTED}
    # vx_attention_cross_f16: the nine (head_dim, waves) instances without a split, both idle-wave forms, the key-range edges, the parts of a split
    one = [c for c in T.CROSS if T.cross_parts(c["Tq"], c["Tk"]) == 1]
    split = [c for c in T.CROSS if T.cross_parts(c["Tq"], c["Tk"]) > 1]
    assert {(c["hd"], T.cross_waves(c["Tq"])) for c in one} == {(hd, nw) for hd in T.CROSS_HD for nw in (1, 2, 4)}
    assert [T.cross_waves(t) for t in (1, 32, 33, 64, 65, 96, 97, 129)] == [1, 1, 2, 2, 4, 4, 4, 4] and [T.cross_parts(*s) for s in ((32, 255), (32, 256), (33, 256), (1, 385))] == [1, 2, 1, 4]
    assert [T.cross_idle_form(t) for t in (64, 65, 96, 97, 128, 129, 257)] == [None, "short", "short", None, None, "last", "last"]
    for hd in T.CROSS_HD:
        mine, mine_split = [c for c in one if c["hd"] == hd], [c for c in split if c["hd"] == hd]
        assert {c["Tq"] for c in mine} >= set(T.CROSS_TQ) and {c["Tk"] for c in mine} >= set(T.CROSS_TK)
        assert {T.cross_idle_form(c["Tq"]) for c in mine} >= {"short", "last"}
        assert {c["Tk"] % 32 for c in mine} >= {0, 1, 31}
        assert {(c["Tq"], c["Tk"]) for c in mine} >= set(T.CROSS_LONG)
        assert {T.cross_parts(c["Tq"], c["Tk"]) for c in mine_split} == {2, 3, 4}
        assert {c["Tk"] for c in mine_split} >= set(T.CROSS_SPLIT_TK) and {c["Tq"] for c in mine_split} >= set(T.CROSS_SPLIT_TQ)
        assert any(c["Tk"] % 128 == 1 for c in mine_split) and any(c["Tk"] % 128 == 0 for c in mine_split)   # a last part of one key, a full last part
        assert any(c["B"] * c["H"] >= 4 and c["B"] > 1 and c["H"] > 1 for c in mine_split)
        assert any(c["mul"] not in (0.0, 1.0) for c in T.CROSS if c["hd"] == hd)
    assert {(c["Tq"], c["Tk"]) for c in one} >= {(tq, tk) for tq in (300, 513) for tk in (1, 7, 32)}
    assert all(c["H"] > 1 for c in T.CROSS) and {c["B"] for c in T.CROSS} == {1, 2, 3}
    assert sum(c["mul"] == 0.0 for c in T.CROSS) >= 3
    kinds = {"random", "spike", "ramp", "low", "vmax"}
    assert {c["data"] for c in one} >= kinds and {c["data"] for c in split} >= kinds
    for c in T.CROSS:   # with fewer queries than keys the queries of the case's problems reach every edge key: attn_cases._cross
        if c["Tq"] < c["Tk"] and c["data"] in ("random", "low", "vmax"):
            assert c["B"] * c["H"] * c["Tq"] >= len(T.cross_edge_keys(c["Tq"], c["Tk"])), c["id"]
    assert T.cross_edge_keys(7, 257) == [0, 31, 32, 63, 64, 95, 96, 127, 128, 159, 160, 191, 192, 223, 224, 255, 256]
    # vx_small_attention_f16: both kernels, both sides of the dispatcher edge, every head_dim on each
    assert {(T.small_few_keys(c), c["hd"]) for c in T.SMALL} == {(f, hd) for f in (True, False) for hd in T.SMALL_HD}
    assert {(c["Nq"], c["Nk"]) for c in T.SMALL} >= set(T.SMALL_SHAPES) and {c["heads"] for c in T.SMALL} == {1, 3}


def _masked_blocks(add):
    """per query: is there a wholly masked 32-key block before its first live key / behind its last one (inside T)"""
    live = np.isfinite(add)
    Tk = add.shape[1]
    nb = Tk // 32 + (Tk % 32 > 0)
    blk = np.stack([live[:, b * 32:(b + 1) * 32].any(1) for b in range(nb)], 1)   # [Tq, blocks]: any live key
    first, last = blk.argmax(1), nb - 1 - blk[:, ::-1].argmax(1)
    return first > 0, last < nb - 1


@pytest.mark.parametrize("case", [c for c in T.MASKED + T.SHIFTED + T.WINDOW], ids=_ids(T.MASKED + T.SHIFTED + T.WINDOW))
def test_masks_leave_every_query_a_key_and_mask_whole_blocks(case):
    a, _ = _made(case["id"])
    before = after = both = False
    for p in R.PROBLEMS[a["entry"]](a):
        assert np.isfinite(p["add"]).any(1).all(), "a query is masked on every key"
        b, f = _masked_blocks(p["add"])
        before, after, both = before or b.any(), after or f.any(), both or (b & f).any()
    if case.get("content") == "band":
        assert both, "no query with wholly masked blocks on both sides of its live keys"
    if case.get("content") == "swin" or case.get("ws", 0) >= 7:
        assert before and after, (before, after)


# ---- 6. the host packers ------------------------------------------------------------------------------------------------------------------------------

def _unpack(packed, N, heads):
    """packed image [heads][QB][QB][64 lanes][16] -> bias [heads, NP, NP] in (query, key) order: the accumulator layout of a 32 x 32 block"""
    QB = T.window_qb(N)
    pk = packed.reshape(heads, QB, QB, 64, 16)
    lane, e = np.meshgrid(np.arange(64), np.arange(16), indexing="ij")
    out = np.full((heads, QB * 32, QB * 32), np.nan, np.float32)
    for qb in range(QB):
        for kb in range(QB):
            out[:, qb * 32 + (lane & 31), kb * 32 + (e >> 2) * 8 + 4 * (lane >> 5) + (e & 3)] = pk[:, qb, kb]
    assert not np.isnan(out).any()
    return out


def _expected_image(bias, N):
    """queries and keys padded to whole blocks: -inf on padded keys, 0 on the live keys of padded queries"""
    NP = T.window_qb(N) * 32
    want = np.zeros((bias.shape[0], NP, NP), np.float32)
    want[:, :N, :N] = bias
    want[:, :, N:] = -np.inf
    return want


@pytest.mark.parametrize("N", [1, 32, 33, 100, 144, 196, 225, 256])
def test_window_bias_packer_is_in_accumulator_order(N):
    lib, heads = L.get_lib(), 2
    rng = np.random.default_rng(N)
    bias = rng.standard_normal((heads, N, N)).astype(np.float16).astype(np.float32)
    bias[rng.random(bias.shape) < 0.1] = -np.inf
    nbytes = lib.vx_window_attention_bias_bytes(N, heads)
    assert nbytes == heads * T.window_qb(N) ** 2 * 64 * 16 * 2
    packed = np.full(nbytes // 2 + 64, 7.0, np.float16)   # a margin behind the image: the packer must leave it alone
    L.vx_check(lib.vx_window_attention_pack_bias(bias.ctypes.data, N, heads, packed.ctypes.data))
    assert (packed[nbytes // 2:] == 7.0).all()
    assert np.array_equal(_unpack(packed[:nbytes // 2].astype(np.float32), N, heads), _expected_image(bias, N))


@pytest.mark.parametrize("ws", [4, 7, 8, 12, 16])
def test_swin_bias_packer_against_the_oracle(ws):
    """four class images: bias, + last-column mask, + last-row mask, + corner mask = the oracle's windows 0 .. 3 of an image of 2 x 2 windows"""
    lib, heads, N = L.get_lib(), 3, ws * ws
    table, bias, masks = T.swin_bias_and_masks(np.random.default_rng(ws), ws, heads, 2, 2)
    img = lib.vx_window_attention_bias_bytes(N, heads) // 2
    packed = np.full(4 * img + 64, 7.0, np.float16)
    L.vx_check(lib.vx_swin_attention_pack_bias(table.ctypes.data, ws, heads, packed.ctypes.data))
    assert (packed[4 * img:] == 7.0).all()
    for cls in range(4):
        got = _unpack(packed[cls * img:(cls + 1) * img].astype(np.float32), N, heads)
        assert np.array_equal(got, _expected_image(bias + masks[cls][None], N)), cls
    assert lib.vx_swin_attention_pack_bias(table.ctypes.data, 17, heads, packed.ctypes.data) == 0 and b"window 17" in lib.vx_last_error()

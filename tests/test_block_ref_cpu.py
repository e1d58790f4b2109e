"""No device: the case table of tests/block_cases.py reaches what it claims, the launcher's refusals precede every HIP call, the two host packers
are bijections, the packed-f16 GELU envelope is what tests/block_ref.py's docstring says, a numpy emulation of the block kernel's arithmetic (its
summation blocks, its f32 LayerNorm, both GELU forms, its rounding points) lies inside the allowance for EVERY case on every buffer, and modelled
wrong kernels lie outside it for some case. No element and no case is exempt anywhere in this file."""
from collections import defaultdict

import numpy as np
import pytest

import block_cases as T
import block_ref as R
from buffer_check import violations
from visioncpp_amd import _lib as L

D, HID, HEADS = R.D, R.HID, R.HEADS
U16, U32 = R.U16, R.U32
BUFFERS = ("x", "cap_x1", "feat", "q", "k", "v")


# ---- 1. the table ------------------------------------------------------------------------------------------------------------------------------

def test_tables_name_what_the_issue_names():
    cases = T.all_cases()
    ids = [c["id"] for c in cases]
    assert len(ids) == len(set(ids)) and len(cases) <= 150 and max(c["M"] for c in cases) <= 400
    # 5 instances x 9 row counts, 7 (M, T) pairs x 2 instances, 3 x 3 scalars + 3 eps on the QKV-only instance, 4 + 2 hidden-unit + 1 + 2 probes
    assert [len(T.group(g)) for g in ("grid", "pairs", "scalars", "probes")] == [45, 14, 12, 9]
    assert set(T.INSTANCES) == {"TTT", "TTF", "TFT", "TFF", "FTF"} and [T.INSTANCES[i] for i in ("TTT", "TTF", "TFT", "TFF", "FTF")] == [
        (True, True, True), (True, True, False), (True, False, True), (True, False, False), (False, True, False)]
    assert T.ROWS == (1, 15, 16, 17, 113, 127, 128, 129, 272)
    assert {(c["inst"], c["M"]) for c in cases} >= {(i, M) for i in T.INSTANCES for M in T.ROWS}       # every instance meets every M
    qkv = [c for c in cases if T.INSTANCES[c["inst"]][1]]
    assert all(c["M"] % c["T"] == 0 for c in qkv)
    for M in T.ROWS:                                                                                    # T = 1 and T = M at every M
        assert {c["T"] for c in qkv if c["M"] == M} >= {1, M}
    assert {(c["M"], c["T"]) for c in qkv} >= {(129, 43), (272, 17), (272, 34), (272, 136), (255, 85), (130, 65), (15, 5)}
    assert any(c["T"] < 16 and c["T"] > 1 for c in qkv)                                                 # q / k / v with an image shorter than a wave
    assert {c["q_scale"] for c in qkv} == {0.125, 1.0, 0.03125} and {c["eps"] for c in cases} == {1e-6, 1e-5, 1e-2}
    assert {(c["q_scale"], c["eps"]) for c in T.group("scalars") if c["inst"] == "TTT"} == {(q, e) for q in T.Q_SCALES for e in T.EPSILONS}
    mlp = [c for c in cases if T.INSTANCES[c["inst"]][0]]
    assert {c["cap"] for c in mlp} == {True, False} and {c["cap"] for c in mlp if c["inst"] == "TTT" and c["wset"] == "dense"} == {True, False}
    # the row classes, mixed inside one call: every class in every wave-sized window of a call of 17 rows and more, every class on varying lanes
    for M in T.ROWS[1:]:
        cls = T.row_classes(M)
        assert set(cls) == set(T.ROW_CLASSES)
        if M >= 32:
            assert all(set(cls[w:w + 16]) >= {"ordinary", "small", "big", "offset", "spike"} for w in range(0, M - 15, 16))
            assert len({m % 16 for m, k in enumerate(cls) if k == "zero"}) >= 2
    c = next(c for c in T.group("scalars"))                                                              # the data the classes promise
    a = T.materialize(c)
    x, att, cls = a["x"][:c["M"]].astype(np.float64), a["att"][:c["M"]].astype(np.float64), np.array(T.row_classes(c["M"]))
    assert not x[cls == "zero"].any() and not att[cls == "zero"].any() and not att[cls == "tiny"].any()
    assert 5e-4 < x[cls == "tiny"].std() < 2e-3 and 100 < x[cls == "big"].std() < 220 and 0.01 < x[cls == "small"].std() < 0.022
    assert 29.5 < x[cls == "offset"].mean() < 30.5 and 0.4 < x[cls == "offset"].std() < 0.6
    assert (np.abs(x[cls == "spike"]).max(axis=1) == 300).all() and ((np.abs(x[cls == "spike"]) > 6).sum(axis=1) == 1).all()
    assert (a["x"][c["M"]:] == T.X_GUARD_VALUE).all() and np.isnan(a["att"][c["M"]:]).all() and not a["vec_mlp"][:D].any()
    want = R.evaluate(a)["_inter"]
    var = want["x1"][cls == "tiny"].var(axis=1)                                                          # eps matters: the variance is about eps
    assert (var > 2e-7).all() and (var < 5e-6).all()
    ftf = R.evaluate(T.materialize(next(c for c in T.group("scalars") if c["inst"] == "FTF")))
    np.testing.assert_allclose(ftf["_inter"]["ln1"][cls == "zero"], np.broadcast_to(T.weights("dense-bo0")["vec_qkv"][D:2 * D], (int((cls == "zero").sum()), D)), rtol=0, atol=0)
    # the probes
    probes = {c["id"]: c for c in T.group("probes")}
    assert all(c["inst"] == "TTT" and c["M"] == 48 for c in probes.values())
    assert {c["s"] for c in probes.values() if c.get("b1") == "sweep"} == {0, 1, 2, 3} and {probes[f"probe-qkv-t{t}"]["T"] for t in (16, 12)} == {16, 12}
    b1, perm = T.sweep_b1()
    assert sorted(perm) == list(range(HID)) and b1.min() == -12 and b1.max() == 12 and len(set(b1.tolist())) == HID
    assert abs(perm[32] - perm[31]) == 1 and abs(perm[1503] - perm[1504]) == 1                             # units 31 / 32 and 1503 / 1504: neighbouring values
    f32_units = np.zeros(HID, bool)
    f32_units[R.F32_UNITS] = True
    assert f32_units.sum() == 64 and np.abs(b1[f32_units]).max() <= 2.1 and np.abs(b1[~f32_units]).max() == 12  # a dense stretch on the f32 units
    for s in (0, 3):                                                                                    # both populations carry every special value
        sp = T.special_b1(s)
        seen = np.zeros(HID, bool)
        seen[384 * s:384 * s + 384] = True
        for v in T.SPECIALS:
            assert (sp[seen & f32_units] == np.float32(v)).any() and (sp[seen & ~f32_units] == np.float32(v)).any(), (s, v)
    assert set(T.SPECIALS) == {0.0, 255.0, -255.0, 256.0, -256.0, 300.0, -300.0, -1000.0, -65504.0, -7.0e4, 6e-8, 6.2e-5}
    for s in range(4):                                                                                  # x out is h[n + 384 s]
        w = T.weights(f"hidden-s{s}")
        assert not w["vec_mlp"][R.V_G2:R.V_B1].any() and not w["vec_mlp"][:D].any() and not w["vec_mlp"][R.V_BFC2:].any()
        n = np.arange(D)
        assert (w["w2"][n, n + 384 * s] == 1).all() and np.count_nonzero(w["w2"]) == D
        a = T.materialize(probes[f"probe-hidden-s{s}"])
        r = R.evaluate(a)
        np.testing.assert_array_equal(r["_inter"]["z"], np.broadcast_to(w["vec_mlp"][R.V_B1:R.V_BFC2].astype(np.float64), (48, HID)))
        np.testing.assert_array_equal(r["x"][0][:48], R.f16(R.gelu_tanh(r["_inter"]["z"]))[:, 384 * s:384 * s + 384])
        # the GELU allowance alone: next to it only the reference's own rounding of h, the nine-term f32 sum and the second-order term of z
        a_h, h, a_z = (r["_inter"][k][:, 384 * s:384 * s + 384] for k in ("a_h", "h", "a_z"))
        assert (r["x"][1][:48] >= a_h).all() and (r["x"][1][:48] <= a_h + (U16 + 10 * U32) * np.abs(h) + R.TINY16 + a_z * a_z / 2).all()
        assert (a_z <= 400 * U32 * np.abs(r["_inter"]["z"][:, 384 * s:384 * s + 384])).all()
    a = T.materialize(probes["probe-outproj"])
    r = R.evaluate(a)
    np.testing.assert_array_equal(r["cap_x1"][0][:48], a["x"][:48].astype(np.float64) + a["att"][:48].astype(np.float64))
    assert np.abs(r["cap_x1"][0]).max() <= 93 and (r["cap_x1"][0] == np.round(r["cap_x1"][0])).all()
    w = T.weights("qkv-onehot")
    assert (np.count_nonzero(w["wqkv"], axis=1) == 1).all() and sorted(set(T.QKV_PERM.tolist())) == list(range(D))
    r = R.evaluate(T.materialize(probes["probe-qkv-t12"]))
    ln16 = R.f16(r["_inter"]["ln1"])
    np.testing.assert_array_equal(r["k"][0][:4].transpose(0, 2, 1, 3).reshape(48, D), ln16[:, T.QKV_PERM[D:2 * D]])
    np.testing.assert_array_equal(r["q"][0][:4].transpose(0, 2, 1, 3).reshape(48, D), 0.03125 * ln16[:, T.QKV_PERM[:D]])
    # the refusals
    fields = [f for f, _ in T.REFUSALS]
    for f in (dict(M=0), dict(x=0), dict(att=0, q=0), dict(w_mlp=0), dict(vec_mlp=0), dict(w_qkv=0), dict(vec_qkv=0), dict(k=0), dict(v=0), dict(T=0), dict(H=0),
              dict(vec_tap=0), dict(att=0), dict(M=1398102, T=1), dict(H=5), dict(H=7), dict(H=12)):
        assert f in fields, f
    assert any(f.get("M", 48) % f.get("T", 16) for f in fields if f.get("T", 16) > 0 and f.get("M", 48) > 0)
    assert 1398102 * D * 4 >= 0x7fffffff > 1398101 * D * 4  # the first M whose x exceeds the buffer range


def test_refusal_table_returns_before_any_launch():
    """host code: every refusal is decided before the first HIP call, so the table runs without a device (the operands are one host buffer)"""
    if L.get_lib().vx_device_count() > 0:
        return  # with a device the GPU suite runs the table, on device memory (a refusal that regressed would launch on these host operands)
    scratch = np.zeros(T.REFUSAL_SCRATCH_BYTES, np.uint8)
    assert T.run_refusals(L.get_lib(), scratch.ctypes.data) == len(T.REFUSALS) == 19
    assert not scratch.any()
    assert b"embed_dim / 64" in L.get_lib().vx_last_error()  # the last entry: H = 12


# ---- 2. the host packers -----------------------------------------------------------------------------------------------------------------------

def test_host_packers_are_bijections():
    """each matrix packed twice, once holding its row indices and once its column indices (raw 16-bit patterns: the packers move halves, they do
    not read them): the pairs read back are every (row, column) of wo | w1 | w2 (of wqkv) exactly once, and every 1 KiB fragment holds 16 rows of
    one 32-wide k-block. The lane order inside a fragment is the probes' business."""
    lib = L.get_lib()

    def indices(rows, cols, row0):
        r = np.ascontiguousarray(np.broadcast_to((np.arange(rows) + row0)[:, None], (rows, cols)).astype(np.uint16))
        c = np.ascontiguousarray(np.broadcast_to(np.arange(cols)[None, :], (rows, cols)).astype(np.uint16))
        return r, c

    mats = [indices(D, D, 0), indices(HID, D, D), indices(D, HID, D + HID)]  # wo, w1, w2; rows numbered through
    n_mlp, n_qkv = lib.vx_dino_block_mlp_bytes() // 2, lib.vx_dino_block_qkv_bytes() // 2
    assert (n_mlp, n_qkv) == (1327104, 442368) == (D * D + 2 * HID * D, 3 * D * D)
    got = []
    for which in (0, 1):
        out = np.full(n_mlp, 0xffff, np.uint16)
        assert lib.vx_dino_block16_pack_mlp(mats[0][which].ctypes.data, mats[1][which].ctypes.data, mats[2][which].ctypes.data, out.ctypes.data) == 1
        got.append(out.astype(np.int64))
    want = np.concatenate([(r.astype(np.int64) * 2048 + c).reshape(-1) for r, c in mats])
    np.testing.assert_array_equal(np.sort(got[0] * 2048 + got[1]), np.sort(want))
    bounds = np.array([0, D, D + HID, 2 * D + HID])

    def fragments(rows, cols, matrix_of=None):
        rows, cols = rows.reshape(-1, 512), cols.reshape(-1, 512)
        assert ((cols // 32).min(axis=1) == (cols // 32).max(axis=1)).all()                     # one 32-wide k-block
        for fr, fc in zip(rows[::37], cols[::37]):                                              # (every 37th in full; the counts for all, below)
            assert len(set(fr.tolist())) == 16 and len(set(zip(fr.tolist(), fc.tolist()))) == 512
        srt = np.sort(rows, axis=1)
        assert ((np.diff(srt, axis=1) != 0).sum(axis=1) == 15).all()                            # 16 distinct rows, 32 halves each
        if matrix_of is not None:
            assert (np.searchsorted(bounds, rows.min(axis=1), "right") == np.searchsorted(bounds, rows.max(axis=1), "right")).all()  # of one matrix

    fragments(got[0], got[1], bounds)
    r, c = indices(3 * D, D, 0)
    got = []
    for m in (r, c):
        out = np.full(n_qkv, 0xffff, np.uint16)
        assert lib.vx_dino_block16_pack_qkv(m.ctypes.data, out.ctypes.data) == 1
        got.append(out.astype(np.int64))
    np.testing.assert_array_equal(np.sort(got[0] * 2048 + got[1]), np.sort((r.astype(np.int64) * 2048 + c).reshape(-1)))
    fragments(got[0], got[1])


# ---- 3. the GELU envelope ----------------------------------------------------------------------------------------------------------------------

def test_packed_f16_gelu_envelope_is_the_figure_of_the_docstring():
    env, at = R.gelu_envelope()
    print(f"\npacked-f16 GELU envelope: {env:.4f} u16 max(|z|, 1) at z = {at:.4f}")
    assert abs(env - R.GELU_ENV_FIGURE) < 0.005, env
    assert f"{R.GELU_ENV_FIGURE:.2f} u16 max(|z|, 1), at z = {at:.2f}" in R.__doc__
    x = np.linspace(-12.0, 12.0, 2400001)  # the two constants of the GELU that the allowance uses: |gelu'| < 1.13, |gelu''| <= 0.8 < 1
    g = R.gelu_grad(x)
    np.testing.assert_allclose(g[1:-1], (R.gelu_tanh(x[2:]) - R.gelu_tanh(x[:-2])) / (x[2:] - x[:-2]), rtol=0, atol=1e-9)
    assert np.abs(g).max() < R.GELU_LIPSCHITZ and np.abs(np.diff(g) / np.diff(x)).max() < 0.8 < R.GELU_CURVATURE
    # what the kernel's comments promise of the sequence at the ends of the range
    for z, want in ((300.0, 300.0), (-300.0, 0.0), (-65504.0, 0.0), (-np.inf, 0.0), (255.0, 255.0), (0.0, 0.0)):
        got = float(R.gelu_f16_sequence(np.array([z], np.float16))[0])
        assert got == want, (z, got)


# ---- 4. a numpy emulation of the kernel's arithmetic, with the defects it can carry -----------------------------------------------------------------

def mm32(a, w, acc):
    """acc + a w^T in f32, the products summed in 32-wide k-blocks, the last block first (the reference sums everything at once in float64)"""
    a, w = a.astype(np.float32), w.astype(np.float32)
    for k in range(a.shape[1] - 32, -1, -32):
        acc = acc + a[:, k:k + 32] @ w[:, k:k + 32].T
    assert acc.dtype == np.float32
    return acc


def ln32(x, g, b, eps, mut):
    """the kernel's LayerNorm: two passes in f32, x * (rstd g) + (b - mean rstd g)"""
    f = np.float32
    mean = x.sum(axis=1, dtype=f, keepdims=True) * f(1.0 / D)
    d = x - mean
    q = (d * d).sum(axis=1, dtype=f, keepdims=True)
    var = q / f(D - 1) if mut == "var_dm1" else q * f(1.0 / D)
    with np.errstate(all="ignore"):
        if mut == "eps_ignored":
            rstd = f(1) / np.sqrt(var)
        elif mut == "eps_outside":
            rstd = f(1) / (np.sqrt(var) + f(eps))
        else:
            rstd = f(1) / np.sqrt(var + f(eps))
        a = rstd * g.astype(f)
        out = x * a + (b.astype(f) - mean * a)
    assert out.dtype == f
    return out


def gelu_device(z, mut):
    """z f32 -> the hidden values (f16): the packed-f16 sequence on units 32 .. 1503, the f32 form on blocks 0 and 47"""
    f = np.float32
    with np.errstate(all="ignore"):
        if mut == "gelu_sigmoid":
            return (z / (f(1) + np.exp(f(-1.702) * z))).astype(np.float16)
        h = R.gelu_f16_sequence(z.astype(np.float16))
        x = z[:, R.F32_UNITS]
        w = x * x * f(f(R.C1) * f(0.044715)) + f(R.C1)
        h[:, R.F32_UNITS] = (x * (f(1) / (f(1) + np.exp2(x * w)))).astype(np.float16)
    return h


def emulate(a, mut=None, guard_rows=R.ROW_GUARD):
    M, T_, eps, qs = a["M"], a["T"], a["eps"], np.float32(a["q_scale"])
    mlp, qkv, tap = R.flags(a)
    f = np.float32
    out = {"x": np.asarray(a["x"], f).reshape(M + guard_rows, D).copy()}
    for n in ("cap_x1", "feat"):
        out[n] = np.zeros((M + guard_rows, D), f)
    x = out["x"][:M].copy()
    if mlp:
        vm = a["vec_mlp"]
        x = mm32(a["att"][:M], a["wo"], x + vm[:D])
        if mut == "stream_f16":
            x = x.astype(np.float16).astype(f)
        if a["cap"]:
            out["cap_x1"][:M] = x
        ln = ln32(x, vm[R.V_G2:R.V_G2 + D], vm[R.V_B2:R.V_B2 + D], eps, mut).astype(np.float16)
        z = mm32(ln, a["w1"], np.broadcast_to(vm[R.V_B1:R.V_BFC2], (M, HID)).astype(f))
        h = gelu_device(z, mut)
        if mut == "block_scaled":
            h[:, 160:192] = (h[:, 160:192].astype(f) * f(0.85)).astype(np.float16)
        if mut == "block0_from_neighbour":
            h[:, :32] = h[:, 32:64]
        if mut == "block47_from_neighbour":
            h[:, HID - 32:] = h[:, HID - 64:HID - 32]
        x = mm32(h, a["w2"], x) + vm[R.V_BFC2:R.V_BFC2 + D]
        out["x"][:M] = x
        if mut == "store_row_M":
            out["x"][M] = x[M - 1]
    if tap:
        out["feat"][:M] = ln32(x, a["vec_tap"][:D], a["vec_tap"][D:], eps, mut).astype(np.float16)
    B = M // T_ if qkv else 1
    for n in "qkv":
        out[n] = np.zeros((B + 1) * HEADS * (T_ if qkv else 1) * 64, f)
    if qkv:
        vq = a["vec_qkv"]
        ln = ln32(x, vq[:D], vq[D:2 * D], eps, mut).astype(np.float16)
        y = mm32(ln, a["wqkv"], np.broadcast_to(vq[2 * D:], (M, 3 * D)).astype(f))
        m = np.arange(M)
        b = (m // 16 * 16) // T_ if mut == "image_from_wave" else m // T_
        tok = m - b * T_
        for i, n in enumerate("qkv"):
            v = y[:, i * D:(i + 1) * D] * (qs if i == 0 or (i == 1 and mut == "k_scaled") else f(1))
            for hd in range(HEADS):
                idx = ((b * HEADS * T_ + tok) * 64 + hd * T_ * 64)[:, None] + np.arange(64)[None, :]
                ok = idx < M * D  # the buffer descriptor ends behind the last image
                out[n][idx[ok]] = v[:, hd * 64:(hd + 1) * 64][ok].astype(np.float16)
        if mut == "guard_image":
            out["v"][M * D + 5] = 1.0
    for n in "qkv":
        out[n] = out[n].reshape(B + 1, HEADS, -1, 64)
    return {n: v.astype(np.float64) for n, v in out.items()}


_CACHE = {}


def _reference(c):
    if c["id"] not in _CACHE:
        a = T.materialize(c)
        _CACHE[c["id"]] = (a, R.evaluate(a))
    return _CACHE[c["id"]]


def _outside(c, mut=None, carried=False):
    """per buffer: elements of the emulation that buffer_check.violations rejects, and the largest error / allowance. As the GPU test does it: x and cap_x1
    against the reference of the inputs, feat / q / k / v against the reference of the stream that came back (`carried`: of the inputs as well,
    with the allowance of x carried into them)"""
    a, ref = _reference(c)
    got = emulate(a, mut)
    if not carried and R.flags(a)[0]:
        ref = dict(ref, **R.evaluate(a, x_out=got["x"]))
    res = {}
    for n in BUFFERS:
        v = violations(got[n], ref[n], untouched=a["x"] if n == "x" else 0.0)  # the GPU test's comparison (a NaN is outside)
        res[n] = (v["stray"] + v["nonfinite"] + v["outside"], v["ratio"])
    return res


def test_emulated_arithmetic_is_inside_the_allowance_for_every_case():
    worst = defaultdict(float)
    for c in T.all_cases():
        for n, (n_bad, ratio) in _outside(c).items():
            assert n_bad == 0, (c["id"], n, n_bad, ratio)
            worst[n] = max(worst[n], ratio)
    print("\nlargest emulated error / allowance per buffer:")
    for k, v in worst.items():
        print(f"  {k:8s} {v:.3f}")
    # no blanket: the emulation's own roundings show in every buffer (cap_x1 is one f32 sum against its (K + 8) u32 worst case)
    assert all(worst[n] > 0.25 for n in ("x", "feat", "q", "k", "v")) and worst["cap_x1"] > 0.01


def _cid(cid):
    return next(c for c in T.all_cases() if c["id"] == cid)


# the modelled wrong kernel -> cases that catch it (each listed case must; a mutant that no case catches means the table or the allowance needs work)
WRONG_KERNELS = [
    ("block_scaled", ["TTT-m1-t1", "TFF-m272-t272", "TFT-m17-t17", "TTT-m33-t11-qs0.125-eps1e-06"]),
    ("block0_from_neighbour", ["probe-hidden-s0", "probe-hidden-special-s0", "TTF-m16-t1", "TFF-m129-t129"]),
    ("block47_from_neighbour", ["probe-hidden-s3", "probe-hidden-special-s3", "TTT-m15-t5", "TFT-m128-t128"]),
    ("var_dm1", ["TTT-m33-t11-qs0.125-eps1e-06", "FTF-m15-t1", "TFT-m1-t1", "probe-qkv-t16"]),
    ("eps_ignored", ["FTF-m33-t11-eps0.01", "FTF-m33-t11-eps1e-06", "TTT-m33-t11-qs1.0-eps1e-05", "TFF-m17-t17", "FTF-m15-t5"]),
    ("eps_outside", ["FTF-m33-t11-eps0.01", "FTF-m33-t11-eps1e-06", "TTT-m33-t11-qs1.0-eps1e-05", "TFF-m17-t17", "FTF-m16-t16"]),
    ("gelu_sigmoid", ["probe-hidden-s0", "probe-hidden-s1", "probe-hidden-s2", "probe-hidden-s3", "TFF-m113-t113", "TTT-m272-t17"]),
    ("stream_f16", ["TTT-m33-t11-qs0.125-eps1e-06", "TFF-m15-t15", "TFT-m1-t1", "TTF-m272-t1"]),
    ("k_scaled", ["TTT-m33-t11-qs0.125-eps1e-06", "probe-qkv-t12", "FTF-m1-t1", "TTF-m16-t1"]),
    ("image_from_wave", ["TTT-m272-t17", "FTF-m15-t5", "probe-qkv-t12", "TTF-m16-t1", "FTF-m272-t136", "TTT-m130-t65", "FTF-m255-t85"]),
    ("store_row_M", ["TTT-m1-t1", "TFF-m128-t128", "TFT-m15-t15", "TTF-m272-t1", "probe-outproj"]),
    ("guard_image", ["FTF-m1-t1", "TTT-m272-t17", "TTF-m128-t1", "FTF-m272-t272"]),
]


@pytest.mark.parametrize("what,ids", WRONG_KERNELS, ids=[w for w, _ in WRONG_KERNELS])
def test_modelled_wrong_kernels_are_outside_the_allowance(what, ids):
    for cid in ids:
        c = _cid(cid)
        assert sum(v[0] for v in _outside(c).values()) == 0, (what, cid)
        assert sum(v[0] for v in _outside(c, what).values()) > 0, (what, cid)


def test_the_allowance_does_not_hide_the_mlp_branch():
    """on the ordinary rows of the dense cases the median allowance of x is at most one eighth of the median |x_out - x1|: a condition that keeps the
    allowance from hiding the branch it is there to check, not a measurement"""
    allow, branch = [], []
    for c in T.dense_cases():
        if not T.INSTANCES[c["inst"]][0]:
            continue
        _, ref = _reference(c)
        rows = np.array(T.row_classes(c["M"])) == "ordinary"
        allow.append(ref["x"][1][:c["M"]][rows].reshape(-1))
        branch.append(np.abs(ref["x"][0][:c["M"]] - ref["_inter"]["x1"])[rows].reshape(-1))
    a, b = np.median(np.concatenate(allow)), np.median(np.concatenate(branch))
    print(f"\nmedian allowance of x {a:.3e}, median |x_out - x1| {b:.3e}: 1 / {b / a:.1f}")
    assert a <= b / 8

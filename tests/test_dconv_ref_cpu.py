"""No device: the float64 reference of vx_dconv3x3_f16 (tests/dconv_ref.py) is pinned to the CPU oracle, a numpy emulation of the kernel's
arithmetic lies inside its allowance, seeded corruptions of that emulation lie outside, vx_dconv_bilinear_supported keeps every halo inside
its source patch, and the case table (tests/dconv_cases.py) covers what the launcher can select."""
import numpy as np
import pytest

import dconv_cases as T
import dconv_ref as R
from oracle import oracle as O
from visioncpp_amd import _lib as L


def _case(**kw):
    base = dict(id="cpu-" + "-".join(f"{k}{v}" for k, v in sorted(kw.items())), B=2, H=9, W=13, cin=64, cout=32, layout="planar")
    base.update(kw)
    return T.materialize(base)


def _result(a, buf):
    """the call's own elements of a flat output buffer -> [B, H, W, n]"""
    B, H, W = a["B"], a["H"], a["W"]
    if a["epi"] == R.DC_RGB_F32:
        return buf[:B * H * W * 3].reshape(B, H, W, 3)
    if a["epi"] == R.DC_HEAD_F32:
        return buf[:B * H * W].reshape(B, H, W, 1)
    return buf[R.out_index(a)]


# ---- 1. the reference against the CPU oracle ---------------------------------------------------------------------------------------------

ORACLE_CASES = [dict(), dict(layout="nhwc", cout=64), dict(up2=1, H=10, W=14), dict(up2=1, H=10, W=14, layout="nhwc", cout=64), dict(a_relu=1, act=2, layout="nhwc"),
                dict(bil=(5, 7), layout="nhwc"), dict(bil=(6, 6), H=10, W=11, layout="nhwc", cin=32), dict(act=1, cin=96, cout=64), dict(cin=32, epi=R.DC_RGB_F32)]


@pytest.mark.parametrize("kw", ORACLE_CASES, ids=[",".join(f"{k}={v}" for k, v in kw.items()) or "plain" for kw in ORACLE_CASES])
def test_reference_matches_the_cpu_oracle(kw):
    a = _case(**kw)
    want, allow, written = R.evaluate(a)
    got = _result(a, want["out"])
    src = R.source_map(a).astype(np.float32)
    if a["bil_hs"] > 0:
        x = O.interpolate_nhwc(src, (a["H"], a["W"]), "bilinear", True)
    elif a["up2"]:
        x = np.repeat(np.repeat(src, 2, axis=1), 2, axis=2)
    else:
        x = src
    if a["a_relu"]:
        x = np.maximum(x, 0)
    w = R.unpack_w(a["w"], a["cin"], a["cout"]).reshape(3, 3, a["cin"], a["cout"]).transpose(3, 0, 1, 2)  # OHWI
    y = O.conv2d_nhwc(np.ascontiguousarray(x, np.float32), np.ascontiguousarray(w, np.float32), a["bias"], stride=1, pad=1).astype(np.float64)
    y = R.activation(y, a["act"])
    if a["epi"] == R.DC_RGB_F32:
        y = y[..., :3]
    # the oracle sums in f32: its own any-order bound, on magnitudes <= |x| (*) |w| + |b| <= 9 cin max|x| max|w| + max|b|
    bound = 2 * (9 * a["cin"] + 8) * R.U32 * (9 * a["cin"] * np.abs(x).max() * np.abs(w).max() + np.abs(a["bias"]).max())
    assert np.abs(got - y).max() <= bound
    assert written["out"].sum() == got.size and (allow["out"][~written["out"]] == 0).all() and (allow["out"][written["out"]] > 0).all()


# ---- 2. / 3. a numpy emulation of the kernel's arithmetic, and corruptions of it --------------------------------------------------------

def f16(x):
    return np.asarray(x, np.float32).astype(np.float16).astype(np.float32)


def lerp2(v, w, f):
    """the kernel's packed-f16 form: fma(f, w, fma(-f, v, v)), each fma rounded to f16 once"""
    t = f16(v.astype(np.float64) - f.astype(np.float64) * v.astype(np.float64))
    return f16(f.astype(np.float64) * w.astype(np.float64) + t.astype(np.float64))


def emulate(a, corrupt=None, seed=0):
    """f16 inputs (bilinear: the lerp2 chain with f16 weights from an f32 table), f32 accumulation of 16-term k-steps in a shuffled order, the
    header's epilogue with an f16 staged tile; `corrupt` plants one defect. Returns the call's elements [B, H, W, n] as float64."""
    rng = np.random.default_rng(seed)
    B, H, W, cin, cout = a["B"], a["H"], a["W"], a["cin"], a["cout"]
    src = R.source_map(a).astype(np.float32)
    if a["bil_hs"] > 0:
        y0, y1, fy = R.bilinear_table(H, a["bil_hs"], np.float32)
        x0, x1, fx = R.bilinear_table(W, a["bil_ws"], np.float32)
        fy, fx = f16(fy)[None, :, None, None], f16(fx)[None, None, :, None]
        p, q, r, s = src[:, y0][:, :, x0], src[:, y0][:, :, x1], src[:, y1][:, :, x0], src[:, y1][:, :, x1]
        x = lerp2(lerp2(p, q, fx), lerp2(r, s, fx), fy)
    else:
        x = src[:, np.arange(H) >> a["up2"]][:, :, np.arange(W) >> a["up2"]]
    raw = x
    if a["a_relu"]:
        x = np.maximum(x, 0)
    if corrupt == "swapped_groups":
        x = x.copy()
        x[..., 8:16], x[..., 16:24] = x[..., 16:24].copy(), x[..., 8:16].copy()
    w9 = R.unpack_w(a["w"], cin, cout).astype(np.float32)
    xp = np.pad(x, ((0, 0), (1, 1), (1, 1), (0, 0)))
    acc = np.zeros((B, H, W, cout), np.float32)
    steps = [(tap, k) for tap in range(9) for k in range(0, cin, 16)]
    for i in rng.permutation(len(steps)):
        tap, k = steps[i]
        ky, kx = divmod(tap, 3)
        win = xp[:, ky:ky + H, kx:kx + W, k:k + 16].copy()
        if corrupt == "halo_shift" and kx == 2 and W > 8:   # the right halo column of the tile that ends at column 8 comes from one pixel further
            win[:, :, 7] = xp[:, ky:ky + H, min(kx + 8, W + 1), k:k + 16]
        if corrupt == "dropped_tap" and tap == 3:           # the left neighbour is missing on the map's top row
            win[:, 0] = 0
        acc = acc + (win @ w9[tap, k:k + 16]).astype(np.float32)
    s1, s2 = np.float32(a["s1"]), np.float32(a["s2"])
    fold = a["x_residual"]
    if fold:
        inv = np.float32(np.float16(np.float32(1) / s1))
        acc[..., :64] += (np.maximum(raw, 0) if corrupt == "fold_relu" else raw)[..., :64] * inv
    v = acc + np.asarray(a["bias"], np.float32)
    if a["epi"] == R.DC_RGB_F32:
        return v[..., :3].astype(np.float64)
    if a["epi"] == R.DC_HEAD_F32:
        dot = (np.maximum(v, 0) * np.asarray(a["head_w"], np.float32)).sum(-1, dtype=np.float32, keepdims=True)
        return (np.maximum(dot + np.float32(a["head_bias"]), 0) * np.float32(a["head_scale"])).astype(np.float64)
    act = (lambda t: np.maximum(t, np.float32(0.2) * t)) if a["act"] == 1 else ((lambda t: np.maximum(t, 0)) if a["act"] == 2 else (lambda t: t))
    r1 = np.asarray(a["res1"])[R.out_index(a, "res1")].astype(np.float32) if a.get("res1") is not None else None
    r2 = np.asarray(a["res2"])[R.out_index(a, "res2")].astype(np.float32) if a.get("res2") is not None else None
    if corrupt == "act_after_residual":
        return f16(act(v + r1)).astype(np.float64)
    v = act(v)
    if fold:
        v = v * s1
    v = f16(v)
    if r1 is not None:
        v = f16(v * s1 + r1)
    if r2 is not None:
        v = f16(v * s2 + r2)
    return v.astype(np.float64)


EMULATED = [dict(act=1), dict(cout=64, res1=1, res2=1, layout="nhwc"), dict(cout=64, res1=1, res2=1, s1=0.2, s2=0.2), dict(cout=64, act=2, res2=1, s2=0.3),
            dict(cout=64, cin=96, x_residual=1, s1=0.2, res2=1, s2=0.2), dict(cout=64, cin=64, x_residual=1, s1=-0.5), dict(bil=(5, 7), layout="nhwc", res1=1),
            dict(bil=(5, 7), layout="nhwc", epi=R.DC_HEAD_F32), dict(cin=32, epi=R.DC_HEAD_F32, layout="nhwc"), dict(epi=R.DC_RGB_F32), dict(up2=1, H=10, W=14, act=1),
            dict(a_relu=1, act=2, layout="nhwc", cout=64)]


@pytest.mark.parametrize("kw", EMULATED, ids=[",".join(f"{k}={v}" for k, v in kw.items()) for kw in EMULATED])
def test_emulated_kernel_arithmetic_is_inside_the_allowance(kw):
    a = _case(**kw)
    want, allow, _ = R.evaluate(a)
    for seed in (0, 1):
        err = np.abs(emulate(a, seed=seed) - _result(a, want["out"]))
        assert (err <= _result(a, allow["out"])).all(), float((err / _result(a, allow["out"])).max())
    # and the allowance is no blanket: about one f16 rounding of the result per rounding step, not a fixed fraction of the largest value
    # (the interpolating loader's worst-case input error, pushed through |w|, is far larger: every input off by its bound in the same direction)
    if a["epi"] == R.DC_F16 and not a["bil_hs"]:
        ratio = _result(a, allow["out"]) / np.maximum(np.abs(_result(a, want["out"])), 0.25)
        assert np.median(ratio) < 6 * R.U16


CORRUPTIONS = [("halo_shift", dict(act=1)), ("dropped_tap", dict(act=1)), ("dropped_tap", dict(epi=R.DC_HEAD_F32, layout="nhwc")), ("swapped_groups", dict(cout=64)),
               ("act_after_residual", dict(act=2, res1=1, cout=64)), ("act_after_residual", dict(act=1, res1=1)),
               ("fold_relu", dict(cout=64, cin=64, x_residual=1, s1=0.2)), ("halo_shift", dict(bil=(5, 7), layout="nhwc"))]


@pytest.mark.parametrize("what,kw", CORRUPTIONS, ids=[f"{w}-{i}" for i, (w, _) in enumerate(CORRUPTIONS)])
def test_seeded_corruptions_are_outside_the_allowance(what, kw):
    a = _case(**kw)
    want, allow, _ = R.evaluate(a)
    clean = np.abs(emulate(a) - _result(a, want["out"])) <= _result(a, allow["out"])
    bad = np.abs(emulate(a, corrupt=what) - _result(a, want["out"])) <= _result(a, allow["out"])
    assert clean.all() and not bad.all(), what


def test_inexact_reciprocal_shows_in_the_fold_term():
    """s1 = 0.3: f16(1 / s1) * s1 is 1.0002, the reference's own term for it is not zero (and the launcher refuses the value)"""
    a = _case(cout=64, cin=64, x_residual=1, s1=0.3)
    exact = R.evaluate(dict(a, s1=0.2))[1]["out"]
    loose = R.evaluate(a)[1]["out"]
    assert np.median(loose[loose > 0]) > 1.05 * np.median(exact[exact > 0])
    ok = L.get_lib().vx_dconv_x_residual_supported
    assert [ok(s, 0, 0) for s in (0.2, 1.0, -0.5, 0.3, 1e-6, 0.0)] == [1, 1, 1, 0, 0, 0]
    assert ok(0.2, 1, 0) == 0 and ok(0.2, 2, 0) == 0 and ok(0.2, 0, 1) == 0


# ---- 4. vx_dconv_bilinear_supported ------------------------------------------------------------------------------------------------------

def _rows_needed(n_out, n_src, halo, stride):
    """for every accepted n_src (an array): the most source rows under one `halo`-row halo that starts at a multiple of `stride` minus 1, from
    the kernel's f32 table: first source row of the halo's first in-map row .. second source row of its last in-map row"""
    first = np.maximum(np.arange(0, n_out, stride) - 1, 0)
    last = np.minimum(np.arange(0, n_out, stride) - 1 + halo - 1, n_out - 1)
    sf = (np.float32(n_out - 1) / (n_src - 1).astype(np.float32))[:, None]

    def i0(o):
        return np.clip(np.floor(o.astype(np.float32)[None, :] / sf).astype(np.int64), 0, n_src[:, None] - 1)
    lo, hi = i0(first), i0(last)
    return (np.minimum(hi + 1, n_src[:, None] - 1) - lo + 1).max(axis=1)


def test_bilinear_supported_keeps_every_halo_inside_its_patch():
    ok = L.get_lib().vx_dconv_bilinear_supported  # host code: loads without a device
    accepted = tight = 0
    tight_pairs = set()
    for n_out in range(2, 1279):
        partner = (3, 2) if n_out + 3 <= 1280 else (2, 2)  # the other axis: the smallest accepted one, none at n_out = 1278
        n_src = np.array([s for s in range(2, n_out + 1) if ok(32, n_out, partner[0], s, partner[1]) and ok(32, partner[0], n_out, partner[1], s)], np.int64)
        if n_src.size == 0:
            continue
        r18, r34 = _rows_needed(n_out, n_src, 18, 16), _rows_needed(n_out, n_src, 34, 32)
        assert (r18 <= 12).all() and (r34 <= 21).all(), (n_out, n_src[(r18 > 12) | (r34 > 21)])
        at_limit = (r18 == 12) | (r34 == 21)
        accepted += n_src.size
        tight += int(at_limit.sum())
        if n_out == T.BIL_TIGHT[0]:
            tight_pairs = set(n_src[at_limit].tolist())
    print(f"{accepted} accepted (n_out, n_src) pairs, {tight} of them need a whole patch")
    assert accepted > 300000 and tight > 10000  # the boundary is real: the closed form is not merely conservative
    assert T.BIL_TIGHT[1] in tight_pairs
    # refusals on either side of each boundary
    assert ok(32, 296, 296, 148, 148) == 1 and ok(64, 296, 296, 148, 148) == 0 and ok(16, 296, 296, 148, 148) == 0
    assert ok(32, 20, 20, 10, 10) == 1 and ok(32, 9, 20, 10, 10) == 0 and ok(32, 20, 9, 10, 10) == 0      # hs > H, ws > W
    assert ok(32, 3, 3, 2, 2) == 1 and ok(32, 3, 3, 1, 2) == 0 and ok(32, 1, 3, 1, 2) == 0
    assert ok(32, 640, 640, 300, 300) == 1 and ok(32, 640, 641, 300, 300) == 0                            # H + W beyond the table
    n = T.BIL_TIGHT[0]
    edge = max(s for s in range(2, n + 1) if ok(32, n, n, s, s))
    assert ok(32, n, n, edge + 1, edge + 1) == 0 and ok(32, n, n, edge, edge + 1) == 0 and ok(32, n, n, edge + 1, edge) == 0  # the scale, per axis
    assert 0.5 < (edge - 1) / (n - 1) < 0.6


# ---- 5. the case table --------------------------------------------------------------------------------------------------------------------

def test_case_table_selects_every_variant_the_launcher_has():
    seen = {}
    for c in T.group("stream") + T.group("stamps"):
        a = T.materialize(dict(c, B=1, H=4, W=4, bil=(2, 2) if c.get("bil") else None))
        v = T.variant_of(a, c.get("res_mode", -1))
        assert v == c["variant"], c["id"]
        assert set(c["caps"]) == {8, 16, 0}
        seen.setdefault(v, set()).add(c["cin"] // 32)
    assert set(seen) == set(T.VARIANTS)
    for v, steps in seen.items():
        one, res = T.VARIANTS[v][7], T.VARIANTS[v][4]
        if one:
            want = {1}
        elif v.endswith("_stamp"):
            want = {3}
        elif res == 2:
            want = {2}               # resident at cin = 64 only
        elif res == 4:
            want = {1, 3, 4}         # cin <= 128; cin = 64 takes RES = 2 whenever the mode allows RES = 4
        elif T.VARIANTS[v][1] == R.DC_HEAD_F32:
            want = {2, 3, 4, 5, 6}   # cin = 32 is the ONE form
        else:
            want = {1, 2, 3, 4, 5, 6}
        assert steps == want, (v, steps)
    assert any(c.get("res_mode", -1) == -1 and c["variant"] == "c32_res4" for c in T.group("stream"))  # the default mode, too


def test_stream_cases_put_a_tile_boundary_on_every_loop_position():
    s = T.STREAM_SHAPE
    tiles = s["B"] * T.tile_count(s["H"], s["W"])
    assert T.tile_count(s["H"], s["W"]) == 8 and tiles == 40
    walks = T.block_tiles(tiles, T.grid_blocks(tiles, 8))
    assert T.grid_blocks(tiles, 8) == 8 and all(len(w) == 5 and w == list(range(w[0], w[0] + 5)) for w in walks)
    assert sorted(t for w in walks for t in w) == list(range(tiles))
    assert any(w[0] // 8 != w[-1] // 8 for w in walks)                                   # a block crosses an image boundary
    assert any({t % 8 for t in w} & {6, 7} and {t % 8 for t in w} & {0, 1} for w in walks)  # and a tile-shape change (tiles 6, 7 of an image are the strip)
    walks16 = T.block_tiles(tiles, T.grid_blocks(tiles, 16))
    assert T.grid_blocks(tiles, 16) == 16 and sorted(t for w in walks16 for t in w) == list(range(tiles)) and all(w[1] - w[0] == 2 for w in walks16)
    assert T.grid_blocks(tiles, 256) == 40 and all(len(w) == 1 for w in T.block_tiles(tiles, 40))
    # ring forms by the period of their unrolled step loop: tile boundaries at step counts k * n, k = 1 .. 4, must hit every position
    hit = {}
    for c in T.group("stream"):
        period = T.unrolled_period(c["variant"])
        n = c["cin"] // 32
        hit.setdefault((period, bool(T.VARIANTS[c["variant"]][6])), set()).update((k * n) % period for k in range(1, 5))
    assert set(hit) == {(6, False), (3, False), (2, False), (2, True)}
    for (period, _), positions in hit.items():
        assert positions == set(range(period)), (period, positions)


def test_case_table_crosses_activations_residuals_and_layouts():
    seen = {(c["cout"], c["act"], bool(c["res1"]), bool(c["res2"]), c["layout"], (c["s1"], c["s2"])) for c in T.group("epilogue") if not c.get("x_residual")}
    assert len(seen) == 2 * 3 * 4 * 2 * 4
    folds = {(c["s1"], bool(c["res2"])) for c in T.group("epilogue") if c.get("x_residual")}
    assert folds == {(s, r) for s in (0.2, 1.0, -0.5) for r in (False, True)}
    geo = T.group("geometry")
    assert {c["W"] for c in geo} >= {1, 15, 16, 17, 31, 32, 33, 48, 49} and {c["H"] for c in geo} >= {1, 15, 16, 17, 31, 32, 33} and {c["B"] for c in geo} >= {1, 3}
    assert {(c["cout"], c["layout"], c["H"]) for c in geo if c.get("up2")} >= {(co, lay, 2) for co in (32, 64) for lay in ("planar", "nhwc")}
    ids = [c["id"] for c in T.all_cases()]
    assert len(ids) == len(set(ids))
    for c in T.all_cases():  # what the launcher's own range checks demand of an accepted call
        assert c["B"] * c["H"] * c["W"] * 64 < 2 ** 22, c["id"]  # small
        if c.get("bil"):
            assert L.get_lib().vx_dconv_bilinear_supported(32, c["H"], c["W"], *c["bil"]) == 1, c["id"]


def test_hooks_validate_their_arguments():
    lib = L.get_lib()
    try:
        assert lib.vx_dconv_set_block_cap(12) == 0 and b"multiple of 8" in lib.vx_last_error()
        assert lib.vx_dconv_set_block_cap(4) == 0
        assert lib.vx_dconv_set_block_cap(8) == 1 and lib.vx_dconv_set_block_cap(16) == 1 and lib.vx_dconv_set_block_cap(-3) == 1
        lib.vx_dconv_set_resident_mode(2)
    finally:
        lib.vx_dconv_set_block_cap(0)
        lib.vx_dconv_set_resident_mode(-1)

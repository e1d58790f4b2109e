"""No device: the restated launchers of tests/head_cases.py agree with the library's host code, the case tables reach what they claim, a numpy
emulation of the head kernels' arithmetic (their rounding points) lies inside the allowance of tests/head_ref.py for EVERY case, and modelled
wrong kernels lie outside it for some case. No element and no case is exempt anywhere in this file."""
from collections import defaultdict

import numpy as np
import pytest

import dconv_ref as D
import head_cases as T
import head_ref as R
from buffer_check import violations
from visioncpp_amd import _lib as L


def f16(x):
    return np.asarray(x, np.float64).astype(np.float16).astype(np.float64)


# ---- 1. the restated host code ------------------------------------------------------------------------------------------------------------

def test_restated_headconv_supported_agrees_with_the_library():
    lib = L.get_lib()
    rng = np.random.default_rng(1)
    n = 0
    for H, W, hs, ws in [tuple(int(v) for v in rng.integers(1, 120, 4)) for _ in range(4000)] + [(c["H"], c["W"], c["hs"], c["ws"]) for c in T.group("headconv")]:
        want = T.headconv_supported(32, 32, H, W, hs, ws)
        assert bool(lib.vx_headconv_supported(32, 32, H, W, hs, ws)) == want, (H, W, hs, ws)
        for cin in (64, 128):
            assert bool(lib.vx_headconv_wide_supported(cin, 32, H, W, hs, ws)) == want
        n += want
    assert n > 200
    assert lib.vx_headconv_supported(64, 32, 17, 33, 10, 19) == 0 and lib.vx_headconv_wide_supported(32, 32, 17, 33, 10, 19) == 0
    assert lib.vx_headconv_supported(32, 64, 17, 33, 10, 19) == 0 and lib.vx_headconv_wide_supported(96, 32, 17, 33, 10, 19) == 0
    # the bound met exactly on either axis, and one source row / column beyond it
    assert T.headconv_supported(32, 32, 18, 40, 10, 5) and 17 * (10 - 1) / (18 - 1) == 9
    assert T.headconv_supported(32, 32, 20, 34, 4, 19) and 33 * (19 - 1) / (34 - 1) == 18
    for _, H, W, hs, ws in T.HEAD_REFUSED_GEOMETRY:
        assert not T.headconv_supported(32, 32, H, W, hs, ws) and lib.vx_headconv_supported(32, 32, H, W, hs, ws) == 0
        assert T.headconv_supported(32, 32, H, W, hs - (hs == 11), ws - (ws == 20))


def test_numpy_packers_are_the_host_packers():
    lib = L.get_lib()
    rng = np.random.default_rng(2)
    for cin in T.CINS:
        Kp = 9 * cin + 32
        rows = np.zeros((32, Kp), np.float16)
        rows[:, :9 * cin] = rng.standard_normal((32, 9 * cin)).astype(np.float16)
        nbytes = lib.vx_headconv_frag_bytes() if cin == 32 else lib.vx_headconv_wide_frag_bytes(cin)
        frag = np.zeros(nbytes // 2, np.float16)
        if cin == 32:
            L.vx_check(lib.vx_headconv_pack(rows.ctypes.data, Kp, frag.ctypes.data))
        else:
            L.vx_check(lib.vx_headconv_wide_pack(rows.ctypes.data, cin, Kp, frag.ctypes.data))
        mine = R.pack_frag(rows, cin)
        np.testing.assert_array_equal(mine.view(np.uint16), frag.view(np.uint16))
        np.testing.assert_array_equal(R.unpack_frag(mine, cin), rows[:, :9 * cin].astype(np.float64).reshape(32, 9, cin).transpose(1, 2, 0))
    w = rng.standard_normal((64, 9, 64)).astype(np.float16)
    np.testing.assert_array_equal(R.unpack_rcu(R.pack_rcu(w)), w.astype(np.float64).transpose(1, 2, 0))
    flat = R.pack_rcu(w).reshape(9, 64, 8, 8)  # the header: group g of row n at position g ^ ((n >> 1) & 7)
    np.testing.assert_array_equal(flat[3, 10, 2 ^ 5], w[10, 3, 16:24])


def test_block_cap_hook_validates_its_argument():
    lib = L.get_lib()
    try:
        assert lib.vx_headconv_set_block_cap(12) == 0 and b"multiple of 8" in lib.vx_last_error()
        assert lib.vx_headconv_set_block_cap(4) == 0 and lib.vx_headconv_set_block_cap(1) == 0
        assert lib.vx_headconv_set_block_cap(8) == 1 and lib.vx_headconv_set_block_cap(16) == 1 and lib.vx_headconv_set_block_cap(-3) == 1
    finally:
        lib.vx_headconv_set_block_cap(0)


def test_refusal_tables_return_before_any_launch():
    """host code: every refusal is decided before the first HIP call, so the tables run without a device (the operands are one host buffer)"""
    if L.get_lib().vx_device_count() > 0:
        return  # with a device the GPU suite runs the tables, on device memory (a refusal that regressed would launch on these host operands)
    scratch = np.zeros(T.REFUSAL_SCRATCH_BYTES, np.uint8)
    assert T.run_refusals(L.get_lib(), scratch.ctypes.data) > 40
    assert not scratch.any()
    kinds = {m for table in (T.HEAD_REFUSALS, T.WIDE_REFUSALS, T.RCU_REFUSALS, T.BIL_REFUSALS) for _, m in table}
    assert {"null operand", "missing operands", "empty batch", "outside the kernel's source patch", "cin 96 (64 or 128)", "C=12 must be a multiple of 8"} <= kinds
    assert any(f == dict(H=T.RCU_HOLE[0], W=T.RCU_HOLE[1]) for f, _ in T.RCU_REFUSALS) and any(f.get("H", 0) > 96 for f, _ in T.RCU_REFUSALS)


def test_capped_walk_reaches_the_steady_state_and_crosses_images():
    c = next(c for c in T.group("headconv") if c["id"] == "head-walk")
    assert c["caps"] == (8, 0) and (c["H"], c["W"], c["hs"], c["ws"], c["B"]) == (64, 96, 36, 54, 3)
    _, _, n_tiles = T.headconv_tiles(c["B"], c["H"], c["W"])
    assert n_tiles == 36 and T.headconv_blocks(n_tiles, 8) == 8
    walks, ranges = T.headconv_walk(n_tiles, 8)
    assert max(len(w) for w in walks) >= 4                                                       # cur ^= 1 more than twice
    assert any(T.tile_image(s, 3, 64, 96) != T.tile_image(t, 3, 64, 96) for w in walks for s, t in zip(w, w[1:]))  # consecutive tiles, two images
    lengths = [hi - lo for lo, hi in ranges]
    assert min(lengths) < max(lengths) and min(lengths) >= 1                                     # one XCD's range is shorter
    assert sorted(t for w in walks for t in w) == list(range(n_tiles))


def test_every_table_walk_visits_every_tile_once():
    for c in T.group("headconv"):
        _, _, n_tiles = T.headconv_tiles(c["B"], c["H"], c["W"])
        if c["cin"] == 32:
            grids = {T.headconv_blocks(n_tiles, cap) for cap in c.get("caps", (0,))} | {T.headconv_blocks(n_tiles, 0, n_cu) for n_cu in (8, 64, 256, 304)}
            for blocks in grids:
                walks, _ = T.headconv_walk(n_tiles, blocks)
                assert sorted(t for w in walks for t in w) == list(range(n_tiles)), (c["id"], blocks)
        else:
            assert sorted(T.headconv_wide_tile(b, n_tiles) for b in range(n_tiles)) == list(range(n_tiles)), c["id"]
    for n_tiles in range(1, 200):  # and in general: any tile count, any multiple of 8 as the cap
        assert sorted(T.headconv_wide_tile(b, n_tiles) for b in range(n_tiles)) == list(range(n_tiles))
        for blocks in {min(n_tiles, cap) for cap in (8, 16, 24, 512)}:
            walks, _ = T.headconv_walk(n_tiles, blocks)
            assert sorted(t for w in walks for t in w) == list(range(n_tiles)), (n_tiles, blocks)


def test_restated_rcu_geometry_and_its_holes():
    lib = L.get_lib()
    refused = set()
    for H in range(1, 97):
        for W in range(1, 97):
            ok = T.rcu_supported(H, W)
            assert bool(lib.vx_rcu_supported(H, W)) == ok, (H, W)
            if not ok:
                refused.add((H, W))
    assert len(refused) == 148 and {(29, 11), (29, 21), (57, 21), (96, 2)} <= refused and T.RCU_HOLE in refused
    for H, W in refused:  # what is refused, as the header says it: a region above 512 pixels or the LDS budget
        g = T.rcu_geometry(H, W)
        assert g["n_in"] > 512 or g["lds"] > T.RCU_LDS_CAP
    assert not any(lib.vx_rcu_supported(H, W) for H, W in ((0, 5), (5, 0), (97, 5), (5, 97), (148, 148), (-1, 3)))
    accepted = T.rcu_accepted()
    assert len({(g["TH"], g["TW"]) for g in (T.rcu_geometry(*hw) for hw in accepted)}) == 751  # distinct tile extents among the accepted maps
    assert T.rcu_geometry(33, 9)["lds"] == 162704 == max(T.rcu_geometry(*hw)["lds"] for hw in accepted) == T.RCU_LDS_CAP - 1136
    table = {(c["H"], c["W"]) for c in T.group("rcu") if c["kind"] == "random" and not c["null"]}
    assert set(T.RCU_FIXED) <= table and all(T.rcu_supported(*hw) for hw in table)
    classes = {T.rcu_class(*hw) for hw in accepted}
    assert len(classes) == 12 and {T.rcu_class(*hw) for hw in table} == classes
    assert {T.rcu_geometry(*hw)["ncx"] for hw in table} == {1, 2, 3, 4, 5} == {T.rcu_geometry(*hw)["ncx"] for hw in accepted}
    for hw in table:
        assert {c["mode"] for c in T.group("rcu") if (c["H"], c["W"]) == hw and c["kind"] == "random" and not c["null"]} == set(T.RCU_MODES)
    for null in (("b1", "b2", "bp"), ("bp",)):
        assert {c["mode"] for c in T.group("rcu") if c["null"] == null} == set(T.RCU_MODES)
    assert {(c["conv"], c["tap"]) for c in T.group("rcu") if c["kind"] == "impulse"} == {(k, t) for k in (1, 2) for t in range(9)}
    assert all(c["B"] == 2 for c in T.group("rcu"))


def test_tables_name_what_the_issue_names():
    head = T.group("headconv")
    geo = {(c["H"], c["W"], c["hs"], c["ws"]) for c in head}
    assert {(3, 3, 2, 2), (16, 32, 9, 17), (17, 33, 10, 19), (40, 72, 2, 2), (48, 40, 5, 23), (47, 70, 27, 40)} <= geo
    for g in T.HEAD_GEOMETRY:
        assert {c["cin"] for c in head if c["id"].startswith(f"head-{g[0]}-")} == set(T.CINS)
    assert {c["B"] for c in head} >= {1, 2, 3}
    assert {(c["cin"], c["slice"], c["tap"]) for c in head if c["kind"] == "impulse"} == {(cin, s, t) for cin in T.CINS for s in range(cin // 32) for t in range(9)}
    assert {(c["cin"], c.get("scale"), c.get("b3")) for c in head if "scale" in c} == {(cin, s, b) for cin in T.CINS for s in (1.0, 2.5, 0.0) for b in (0.3, -0.3)}
    assert {c["kind"] for c in head} == {"random", "positive", "impulse", "negative", "large"}
    for g in T.HEAD_GEOMETRY:  # every geometry, and the walk, with data that makes the allowance sharp, at every cin
        assert {c["cin"] for c in head if c["id"].startswith(f"head-{g[0]}-") and c["kind"] == "positive"} == set(T.CINS)
    assert {c["cin"] for c in head if c["id"].startswith("head-walk") and c["kind"] == "positive"} == set(T.CINS)
    assert {(c["cin"], c["at"], c["tap"]) for c in head if c["kind"] == "impulse"} == {(cin, at, t) for cin in T.CINS for at in T.IMPULSE_AT for t in range(9)}
    for at, (geo, sy, sx) in T.IMPULSE_AT.items():  # where the impulses sit: the four corners' and edges' source pixels, and under both tile seams
        oy, ox = (sy % geo["hs"]) * (geo["H"] - 1) / (geo["hs"] - 1), (sx % geo["ws"]) * (geo["W"] - 1) / (geo["ws"] - 1)
        if at == "seam":
            assert 14 < oy < 17 and 31 < ox < 33 and geo["H"] > 17 and geo["W"] > 33
        elif at != "centre":
            assert oy in (0, geo["H"] - 1) or ox in (0, geo["W"] - 1)
    # full-patch: the kernel's f32 table needs all 12 source rows under some tile's 18 halo rows and all 21 columns under some 34
    g = next(g for g in T.HEAD_GEOMETRY if g[0] == "full-patch")
    for n_out, n_src, tile, patch in ((g[1], g[3], 16, 12), (g[2], g[4], 32, 21)):
        i0 = D.bilinear_table(n_out, n_src, np.float32)[0]
        need = max(min(i0[min(t + tile, n_out - 1)] + 1, n_src - 1) - i0[max(t - 1, 0)] + 1 for t in range(0, n_out, tile))
        assert need == patch, (n_out, n_src, need)
    bil = T.group("bilinear")
    assert {c["C"] for c in bil} == {8, 24, 64}
    assert any((c["H"], c["W"]) == (c["OH"], c["OW"]) for c in bil) and any(c["H"] == 1 and c["OH"] > 1 for c in bil) and any(c["OH"] == 1 and c["H"] > 1 for c in bil)
    assert any(c["OH"] * 2 == c["H"] and c["OW"] * 2 == c["W"] for c in bil) and any(c["OH"] == 2 * c["H"] for c in bil)
    assert any(c["OW"] * c["C"] // 8 > 256 and (c["OW"] * c["C"] // 8) % 256 for c in bil)
    ids = [c["id"] for c in T.all_cases()]
    assert len(ids) == len(set(ids))
    for c in T.all_cases():  # no shape above what the issue allows
        assert (c["H"] <= 96 and c["W"] <= 96) if c["entry"] == "rcu" else c["B"] * c.get("OH", c["H"]) * c.get("OW", c["W"]) <= 3 * 64 * 96
    for c in T.group("headconv") + T.group("rcu"):
        if c["kind"] == "negative":  # whole regions exactly zero, and not everything
            want, allow, _ = R.headconv(T.materialize(c))
            assert 0.3 < (want == 0).mean() < 0.7 and (allow[want == 0] == 0).all() and (allow[want > 0] > 0).all(), c["id"]  # the zero region is compared exactly
        if c["kind"] == "large":     # a few hundred, and the reference's own intermediates stay finite in f16
            a = T.materialize(c)
            want, _, inter = (R.headconv if c["entry"] == "headconv" else R.rcu)(a)
            assert all(np.abs(v).max() < 65504 for v in inter.values()) and np.abs(want).max() < 65504 and max(np.abs(v).max() for v in inter.values()) > 300, c["id"]


def test_impulse_references_are_the_known_footprints():
    for c in T.group("headconv"):
        if c["kind"] != "impulse":
            continue
        a = T.materialize(c)
        want = R.headconv(a)[0]
        src = np.zeros((1, c["hs"], c["ws"], 1))
        _, sy, sx = T.IMPULSE_AT[c["at"]]
        src[0, sy % c["hs"], sx % c["ws"], 0] = 1.5
        up = np.pad(R.resize(src, c["H"], c["W"])[0][0, :, :, 0], 1)
        ky, kx = divmod(c["tap"], 3)
        np.testing.assert_allclose(want[-1], up[ky:ky + c["H"], kx:kx + c["W"]], rtol=0, atol=1e-12)  # out(y, x) = in(y + ky - 1, x + kx - 1)
        assert not want[:-1].any() and want[-1].any()
    for c in T.group("rcu"):
        if c["kind"] != "impulse":
            continue
        want = R.rcu(T.materialize(c))[0]
        H, W, tap = c["H"], c["W"], c["tap"]
        ky, kx = divmod(tap, 3)
        ch, n = (5 * tap + 2) % 64, (11 * tap + 7) % 64
        exp = np.zeros((H, W, 64))
        exp[H // 2, W // 2, ch] += 1.5                # + x (and, for an impulse of conv 2, conv1 = identity feeds it)
        exp[H // 2 + 1 - ky, W // 2 + 1 - kx, n] += 1.5
        np.testing.assert_allclose(want[-1], exp, rtol=0, atol=1e-12)
        assert not want[0].any()


# ---- 2. numpy emulations of the kernels' arithmetic, with the defects they can carry -------------------------------------------------------

def lerp2(v, w, f):
    """packed halves, uncontracted: every operation of f * w + (v - f * v) rounded to f16"""
    return f16(f16(f * w) + f16(v - f16(f * v)))


def _acc_conv(x, w9, step=16):
    """f32 accumulation of 16-term k-steps, tap by tap; x, w9 hold f16 values"""
    B, H, W, cin = x.shape
    xp = np.pad(x, ((0, 0), (1, 1), (1, 1), (0, 0))).astype(np.float32)
    w = w9.astype(np.float32)
    acc = np.zeros((B, H, W, w9.shape[2]), np.float32)
    for k in range(0, cin, step):
        for tap in range(9):
            ky, kx = divmod(tap, 3)
            acc = acc + xp[:, ky:ky + H, kx:kx + W, k:k + step] @ w[tap, k:k + step]
    return acc


def emulate_headconv(a, corrupt=None):
    B, H, W, hs, ws, cin = (a[k] for k in ("B", "H", "W", "hs", "ws", "cin"))
    flat = np.asarray(a["x"]).astype(np.float64)
    src = flat[:B * hs * ws * cin].reshape(B, hs, ws, cin)
    y0, y1, fy = D.bilinear_table(H, hs, np.float32)
    x0, x1, fx = D.bilinear_table(W, ws, np.float32)
    fy, fx = f16(fy)[None, :, None, None], f16(fx)[None, None, :, None]
    rows = src
    if corrupt == "has_next_ignored":   # the second row is i0 + 1 whatever the map's extent: behind an image's last row lies the next image, then the NaN tail
        tail = np.full(ws * cin, np.nan)
        tail[:min(tail.size, flat.size - src.size)] = flat[src.size:src.size + tail.size]
        after = np.concatenate([src[1:, :1], tail.reshape(1, 1, ws, cin)])
        rows = np.concatenate([src, after], axis=1)
        y1 = y0 + 1
    if corrupt == "clamped_row_weighted":  # the patch fill clamps one row early: a repeated row stands where the map's last row should carry weight
        y0, y1 = np.minimum(y0, hs - 2), np.minimum(y1, hs - 2)
    p, q, r, s = rows[:, y0][:, :, x0], rows[:, y0][:, :, x1], rows[:, y1][:, :, x0], rows[:, y1][:, :, x1]
    halo = lerp2(lerp2(p, q, fx), lerp2(r, s, fx), fy)
    halo_b = None
    if corrupt in ("patch_row_short", "patch_col_short"):
        # the patch's 12th row (21st column) repeats the one before although the map has one: a clamped row carries weight, with real values. Only
        # a tile's last halo row (column) reaches that far, so the outputs next to the seam below (right of) it see it: `halo_b` is the halo as the
        # tiles above (left of) the seams hold it
        yb0, yb1, xb0, xb1 = y0.copy(), y1.copy(), x0.copy(), x1.copy()
        if corrupt == "patch_row_short":
            for o in range(16, H, 16):
                limit = y0[max(o - 17, 0)] + 10
                yb0[o], yb1[o] = min(y0[o], limit), min(y1[o], limit)
        else:
            for o in range(32, W, 32):
                limit = x0[max(o - 33, 0)] + 19
                xb0[o], xb1[o] = min(x0[o], limit), min(x1[o], limit)
        halo_b = lerp2(lerp2(rows[:, yb0][:, :, xb0], rows[:, yb0][:, :, xb1], fx), lerp2(rows[:, yb1][:, :, xb0], rows[:, yb1][:, :, xb1], fx), fy)
    if corrupt == "rim_row_wrong":     # the map's top row holds the second row's values
        halo[:, 0] = halo[:, 1]
    if corrupt == "seam_column_wrong":  # the first column behind the x = 32 tile seam holds its left neighbour's values
        halo[:, :, 32] = halo[:, :, 31]
    if corrupt == "slices_reversed":
        halo = halo.reshape(B, H, W, cin // 32, 32)[:, :, :, ::-1].reshape(B, H, W, cin)
    w9 = R.unpack_frag(a["wfrag"], cin)
    if corrupt == "taps_transposed":
        w9 = w9.reshape(3, 3, cin, 32).transpose(1, 0, 2, 3).reshape(9, cin, 32)
    if corrupt == "halo_not_zero":      # positions outside the map hold the nearest map value instead of zero
        xp = np.pad(halo, ((0, 0), (1, 1), (1, 1), (0, 0)), mode="edge").astype(np.float32)
        acc = np.zeros((B, H, W, 32), np.float32)
        for k in range(0, cin, 16):
            for tap in range(9):
                ky, kx = divmod(tap, 3)
                acc = acc + xp[:, ky:ky + H, kx:kx + W, k:k + 16] @ w9[tap, k:k + 16].astype(np.float32)
    else:
        acc = _acc_conv(halo, w9)
    if halo_b is not None:
        acc_b = _acc_conv(halo_b, w9)
        if corrupt == "patch_row_short":
            acc[:, 15::16] = acc_b[:, 15::16]
        else:
            acc[:, :, 31::32] = acc_b[:, :, 31::32]
    v = np.maximum(acc + np.asarray(a["bias"], np.float32), np.float32(0))
    dot = np.zeros((B, H, W), np.float32)
    for n in range(32):
        dot = dot + v[..., n] * np.float32(a["w3"][n])
    if corrupt != "b3_dropped":
        dot = dot + np.float32(a["b3"])
    if corrupt != "last_relu_dropped":
        dot = np.maximum(dot, np.float32(0))
    if corrupt == "all_zeros":
        dot = dot * np.float32(0)
    return (np.float32(a["scale"]) * dot).astype(np.float64)


def emulate_rcu(a, corrupt=None):
    B, H, W = a["B"], a["H"], a["W"]
    x = np.asarray(a["x"]).astype(np.float64)[:B * H * W * 64].reshape(B, H, W, 64)
    garbage = np.full(64, 0.37, np.float32) if corrupt == "null_bias_garbage" else np.zeros(64, np.float32)
    b1, b2, bp = (garbage if a.get(k) is None else np.asarray(a[k], np.float32) for k in ("b1", "b2", "bp"))
    w1, w2 = R.unpack_rcu(a["w1"]), R.unpack_rcu(a["w2"])
    xe = np.pad(np.maximum(x, 0), ((0, 0), (1, 1), (1, 1), (0, 0)))  # conv1 over the map and its one-pixel rim
    mid = f16(np.maximum(_acc_conv(xe, w1) + b1, np.float32(0)))
    if corrupt != "rim_not_zeroed":
        mid[:, 0], mid[:, -1], mid[:, :, 0], mid[:, :, -1] = 0, 0, 0, 0
    c2 = _acc_conv(mid, w2)[:, 1:-1, 1:-1]  # (its own zero padding lies outside the rim: never inside an in-map window)
    v = f16(c2 + b2)
    v = f16(v + (np.roll(x, 1, axis=2) if corrupt == "x_off_by_one" else x))
    if a.get("res2") is not None:
        v = f16(v + np.asarray(a["res2"]).astype(np.float64).reshape(x.shape))
    if a.get("wp") is not None:
        wp = R.unpack_rcu(a["wp"])[0].astype(np.float32)
        acc = np.zeros((B, H, W, 64), np.float32)
        for k in range(0, 64, 16):
            acc = acc + v[..., k:k + 16].astype(np.float32) @ wp[k:k + 16]
        v = f16(acc + bp)
    if corrupt == "second_mtile_skipped":  # the pixels of a tile's M-tiles 8 .. 15 (flat index 256 and up) keep the buffer's zeros
        g = T.rcu_geometry(H, W)
        pd = (np.arange(H) % g["TH"])[:, None] * g["TW"] + (np.arange(W) % g["TW"])[None, :]
        v = np.where((pd >= 256)[None, :, :, None], 0.0, v)
    return v


def emulate_bilinear(a, corrupt=None):
    B, H, W, C, OH, OW = (a[k] for k in ("B", "H", "W", "C", "OH", "OW"))
    src = np.asarray(a["x"]).astype(np.float32)[:B * H * W * C].reshape(B, H, W, C)
    y0, y1, dy = D.bilinear_table(OH, H, np.float32)
    x0, x1, dx = D.bilinear_table(OW, W, np.float32)
    dy, dx = dy[None, :, None, None], dx[None, None, :, None]
    one = np.float32(1)
    w00, w01, w10, w11 = (one - dx) * (one - dy), dx * (one - dy), (one - dx) * dy, dx * dy
    v = src[:, y0][:, :, x0] * w00 + src[:, y0][:, :, x1] * w01 + src[:, y1][:, :, x0] * w10 + src[:, y1][:, :, x1] * w11
    assert v.dtype == np.float32
    return f16(v)


EMULATE = {"headconv": emulate_headconv, "rcu": emulate_rcu, "bilinear": emulate_bilinear}
REF = {"headconv": R.headconv, "rcu": R.rcu, "bilinear": R.bilinear}
_CACHE = {}


def _reference(c):
    if c["id"] not in _CACHE:
        a = T.materialize(c)
        _CACHE[c["id"]] = (a,) + REF[c["entry"]](a)[:2]
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
        key = c["entry"] + ("" if c["entry"] != "headconv" else f"-cin{c['cin']}")
        worst[key] = max(worst[key], ratio)
        if c["entry"] == "headconv":
            worst["headconv/" + c["kind"]] = max(worst["headconv/" + c["kind"]], ratio)
    print("\nlargest emulated error / allowance per entry point:")
    for k, v in sorted(worst.items()):
        print(f"  {k:16s} {v:.3f}")
    # the allowance is no blanket where a result is rounded to f16 on the way out (headconv's is its worst case: every halo value off by its
    # bound in the same direction, pushed through |w|; the wrong kernels below show that it still separates)
    assert worst["rcu"] > 0.25 and worst["bilinear"] > 0.25
    # headconv: the bound is linear in sum |x| |w| |w3| with every halo value off by 10 u16 in one direction, where real roundings are 8 of at
    # most u16 / 2 each with random signs, averaged over the 9 cin terms of a sum: of the order of a per cent of it on the data without
    # cancellation -- a multiple of the share that zero-mean data reaches
    assert worst["headconv/positive"] > 0.008 and worst["headconv/negative"] > 0.005 and 2 * worst["headconv/random"] < worst["headconv/positive"]


def _case(cid):
    return next(c for c in T.all_cases() if c["id"] == cid)


def _two_out_case():
    return next(c for c in T.group("rcu") if c["kind"] == "random" and c["mode"] == "rcu" and not c["null"] and T.rcu_class(c["H"], c["W"])[1])


WRONG_KERNELS = [
    ("taps_transposed", ["head-impulse-cin32-s0-tap1", "head-impulse-cin128-s3-tap5", "head-ragged-cin64-pos", "head-bound-y-cin32-pos", "head-impulse-cin64-seam-tap2"]),
    ("has_next_ignored", ["head-second-tile-cin32", "head-sub-tile-cin128"]),
    ("clamped_row_weighted", ["head-sub-tile-cin32-pos", "head-upscale-cin64-pos", "head-bound-y-cin32-pos", "head-impulse-cin32-bottom-tap4"]),
    ("patch_row_short", ["head-full-patch-cin32-pos", "head-full-patch-cin128-pos"]),
    ("patch_col_short", ["head-full-patch-cin32-pos", "head-full-patch-cin64-pos"]),
    ("rim_row_wrong", ["head-ragged-cin32-pos", "head-bound-y-cin64-pos", "head-sub-tile-cin128-pos", "head-impulse-cin32-top-tap4"]),
    ("seam_column_wrong", ["head-ragged-cin32-pos", "head-second-tile-cin64-pos", "head-anisotropic-cin128-pos", "head-impulse-cin32-seam-tap4"]),
    ("halo_not_zero", ["head-one-tile-cin64-pos", "head-sub-tile-cin32-pos", "head-impulse-cin32-corner00-tap0", "head-impulse-cin128-corner11-tap8"]),
    ("slices_reversed", ["head-impulse-cin64-s0-tap4", "head-impulse-cin128-s1-tap4", "head-second-tile-cin128-pos", "head-ragged-cin64-pos"]),
    ("b3_dropped", ["head-scale1-b3+0.3-cin32", "head-scale2.5-b3-0.3-cin64", "head-ragged-cin32-pos"]),
    ("last_relu_dropped", ["head-negative-cin32", "head-negative-cin128"]),
    ("all_zeros", ["head-negative-cin32", "head-negative-cin64", "head-ragged-cin32-pos"]),
    ("taps_transposed_rcu", ["rcu-impulse-conv1-tap1", "rcu-impulse-conv2-tap5"]),
    ("rim_not_zeroed", ["rcu-1x1-rcu", "rcu-1x96-rcu+res+proj"]),
    ("x_off_by_one", ["rcu-33x9-rcu", "rcu-1x96-rcu+proj"]),
    ("null_bias_garbage", ["rcu-nobias-rcu", "rcu-nobias-rcu+res+proj", "rcu-nobp-rcu+proj"]),
    ("second_mtile_skipped", [None]),
]


def test_has_next_guards_against_non_finite_memory_only():
    """With align_corners the weight of the second source row is 0 (or one f32 rounding away from it) wherever has-next is 0, so ignoring the
    flag moves no finite result: the defect shows only where the memory behind the map is not finite, which is why every source tensor of the
    table ends in NaNs. Pinned here so that nobody takes the flag's test for a test of values."""
    c = _case("head-second-tile-cin32-pos")
    a, want, allow = _reference(c)
    finite = dict(a, x=np.concatenate([a["x"][:-T.NAN_TAIL], np.full(a["ws"] * a["cin"], 60000.0, np.float16)]))
    err = np.abs(emulate_headconv(finite, "has_next_ignored") - want)
    assert (err <= allow).all()  # (60000 x a weight of at most one f32 rounding of the coordinate, or the next image's row x the same)
    assert (np.abs(emulate_headconv(a, "has_next_ignored") - want) <= allow).sum() < want.size


@pytest.mark.parametrize("what,ids", WRONG_KERNELS, ids=[w for w, _ in WRONG_KERNELS])
def test_modelled_wrong_kernels_are_outside_the_allowance(what, ids):
    for cid in ids:
        c = _two_out_case() if cid is None else _case(cid)
        if what == "taps_transposed_rcu":
            a, want, allow = _reference(c)
            swap = lambda flat: R.pack_rcu(R.unpack_rcu(flat).reshape(3, 3, 64, 64).transpose(1, 0, 3, 2).reshape(9, 64, 64).transpose(1, 0, 2))  # noqa: E731
            wrong = dict(a, w1=swap(a["w1"]), w2=swap(a["w2"]))
            assert (np.abs(emulate_rcu(a) - want) <= allow).all() and not (np.abs(emulate_rcu(wrong) - want) <= allow).all(), cid
            continue
        assert _outside(c)[0] == 0, (what, c["id"])
        assert _outside(c, what)[0] > 0, (what, c["id"])

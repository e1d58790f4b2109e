"""The case tables of the Depth-Anything head kernels' argument space -- vx_headconv_bil_f16, vx_headconv_wide_bil_f16, vx_rcu_fused_f16,
vx_bilinear_ac_f16 -- built the same way by the CPU tests that check their completeness (tests/test_head_ref_cpu.py) and by the GPU tests that
run them (tests/test_gpu_head_matrix.py). A case is a small dict; `materialize` turns it into the `args` dict of tests/head_ref.py, seeded by
the case id. The launchers' host-side decisions are restated here from csrc/kernels_headconv.hip and csrc/kernels_rcu.hip, so that the tables
can be checked against them without a device."""
from __future__ import annotations

import zlib

import numpy as np

import head_ref as R

# ---- the launchers, restated ----------------------------------------------------------------------------------------------------------------

TH, TW, PR, PC = 16, 32, 12, 21  # the head kernels' output tile and source patch


def headconv_supported(cin, cout, H, W, hs, ws) -> bool:
    """vx_headconv_supported at cin 32, vx_headconv_wide_supported at 64 / 128"""
    if cin not in (32, 64, 128) or cout != 32 or H < 2 or W < 2 or hs < 2 or ws < 2:
        return False
    sy, sx = (hs - 1) / (H - 1), (ws - 1) / (W - 1)
    return int(17 * sy) + 3 <= PR and int(33 * sx) + 3 <= PC


def headconv_tiles(B, H, W):
    tx, ty = (W + TW - 1) // TW, (H + TH - 1) // TH
    return tx, ty, tx * ty * B


def headconv_blocks(n_tiles, cap=0, n_cu=256) -> int:
    """the 32-channel launcher's grid: two persistent blocks per CU, or the test hook's cap"""
    return min(n_tiles, cap if cap > 0 else 2 * n_cu)


def headconv_walk(n_tiles, blocks):
    """the 32-channel kernel: the tiles block `id` visits, in order, and every XCD's tile range"""
    per_xcd_tiles = (n_tiles + 7) >> 3
    walks, ranges = [], []
    for xcd in range(8):
        t_begin = xcd * per_xcd_tiles
        ranges.append((t_begin, max(t_begin, min(t_begin + per_xcd_tiles, n_tiles))))
    for i in range(blocks):
        xcd, in_xcd = i & 7, i >> 3
        per_xcd_blocks = (blocks + 7 - xcd) >> 3
        t_begin, t_end = ranges[xcd]
        walks.append(list(range(t_begin + in_xcd, t_end, per_xcd_blocks)))
    return walks, ranges


def headconv_wide_tile(block, blocks) -> int:
    """the wide kernel: the one tile of block `block` of a grid of `blocks` (= the tile count)"""
    q, rem, xcd = blocks >> 3, blocks & 7, block & 7
    return (xcd * (q + 1) if xcd < rem else rem * (q + 1) + (xcd - rem) * q) + (block >> 3)


def tile_image(t, B, H, W):
    tx, ty, _ = headconv_tiles(B, H, W)
    return t // (tx * ty)


def rcu_geometry(H, W) -> dict:
    ncx = (W + 19) // 20
    tw = (W + ncx - 1) // ncx
    th = min(320 // tw, H)
    ncy = (H + th - 1) // th
    th = (H + ncy - 1) // ncy
    g = dict(TH=th, TW=tw, ncx=ncx, ncy=ncy, n_in=(th + 4) * (tw + 4), n_mid=(th + 2) * (tw + 2), n_out=th * tw)
    g["lds"] = (g["n_in"] + ((g["n_mid"] + 31) & ~31)) * 144 + 4 * (64 * 64 * 2) + 3 * 64 * 4
    return g


RCU_LDS_CAP = 160 * 1024


def rcu_supported(H, W) -> bool:
    if H < 1 or W < 1 or H > 96 or W > 96:
        return False
    g = rcu_geometry(H, W)
    return g["n_in"] <= 512 and g["n_mid"] <= 512 and g["n_out"] <= 512 and g["lds"] <= RCU_LDS_CAP


def rcu_class(H, W):
    """(a wave owns two M-tiles of the intermediate, two of the output, the last tile column is ragged, the last tile row is ragged)"""
    g = rcu_geometry(H, W)
    return ((g["n_mid"] + 31) // 32 > 8, (g["n_out"] + 31) // 32 > 8, g["ncx"] * g["TW"] != W, g["ncy"] * g["TH"] != H)


def rcu_accepted():
    return [(H, W) for H in range(1, 97) for W in range(1, 97) if rcu_supported(H, W)]


# ---- headconv cases ---------------------------------------------------------------------------------------------------------------------------

CINS = (32, 64, 128)
# (name, H, W, hs, ws, B): every geometry runs at every cin
HEAD_GEOMETRY = [
    ("sub-tile", 3, 3, 2, 2, 2),          # a map smaller than one tile on a source smaller than the patch
    ("one-tile", 16, 32, 9, 17, 1),
    ("second-tile", 17, 33, 10, 19, 3),   # one row and one column into the second tile
    ("bound-y", 18, 40, 10, 5, 1),        # 17 sy = 9 exactly
    ("bound-x", 20, 34, 4, 19, 2),        # 33 sx = 18 exactly
    ("upscale", 40, 72, 2, 2, 1),
    ("anisotropic", 48, 40, 5, 23, 2),
    ("ragged", 47, 70, 27, 40, 3),        # the production ratio
    ("full-patch", 34, 66, 20, 38, 2),    # some tile needs all 12 source rows, some all 21 columns (asserted by the CPU test)
]
HEAD_REFUSED_GEOMETRY = [("beyond-y", 18, 40, 11, 5), ("beyond-x", 20, 34, 4, 20)]  # one source row / column beyond the bound
SMALL = dict(H=17, W=33, hs=10, ws=19)    # four tiles, every one of them ragged or not: the shape of the data-kind cases
SEAM = dict(H=24, W=48, hs=13, ws=26)     # source pixel (8, 17) lies under output (15.3, 32.0): its footprint crosses the y = 16 and x = 32 tile seams
# where an impulse sits: (geometry, source row, source column), negative = from the end
IMPULSE_AT = {"centre": (SMALL, 5, 9), "corner00": (SMALL, 0, 0), "corner11": (SMALL, -1, -1), "top": (SMALL, 0, 9), "bottom": (SMALL, -1, 9),
              "left": (SMALL, 5, 0), "right": (SMALL, 5, -1), "seam": (SEAM, 8, 17)}
WALK = dict(H=64, W=96, hs=36, ws=54, B=3, cin=32)  # 36 tiles: 12 per image
WALK_CAP = 8


def _head_cases():
    """`positive` and `negative` data have no cancellation (x, w, w3 >= 0), so the derived allowance is about 1 % of an element: every geometry and
    the walk run with it at every cin; `random` (zero mean: the allowance is a large share of the output) stays for the signs"""
    out = []
    for name, H, W, hs, ws, B in HEAD_GEOMETRY:
        for cin in CINS:
            for kind in ("positive", "random"):
                out.append(dict(id=f"head-{name}-cin{cin}" + ("" if kind == "random" else "-pos"), entry="headconv", kind=kind, cin=cin, B=B, H=H, W=W, hs=hs, ws=ws))
    for cin in CINS:
        for s in range(cin // 32):
            for tap in range(9):
                out.append(dict(SMALL, id=f"head-impulse-cin{cin}-s{s}-tap{tap}", entry="headconv", kind="impulse", cin=cin, B=2, slice=s, tap=tap, at="centre"))
        for at, (geo, _, _) in IMPULSE_AT.items():  # the rims, the corners, the last source row / column, the tile seams: the last slice, every tap
            if at != "centre":
                for tap in range(9):
                    out.append(dict(geo, id=f"head-impulse-cin{cin}-{at}-tap{tap}", entry="headconv", kind="impulse", cin=cin, B=2, slice=cin // 32 - 1, tap=tap, at=at))
        out.append(dict(SMALL, id=f"head-negative-cin{cin}", entry="headconv", kind="negative", cin=cin, B=2))
        out.append(dict(SMALL, id=f"head-large-cin{cin}", entry="headconv", kind="large", cin=cin, B=2))
        for scale in (1.0, 2.5, 0.0):
            for b3 in (0.3, -0.3):
                out.append(dict(SMALL, id=f"head-scale{scale:g}-b3{b3:+g}-cin{cin}", entry="headconv", kind="positive", cin=cin, B=1, scale=scale, b3=b3))
    out.append(dict(WALK, id="head-walk", entry="headconv", kind="positive", caps=(WALK_CAP, 0)))
    for cin in (64, 128):
        out.append(dict(WALK, id=f"head-walk-cin{cin}", entry="headconv", kind="positive", cin=cin))
    return out


# ---- rcu cases ------------------------------------------------------------------------------------------------------------------------------

RCU_MODES = {"rcu": (0, 0), "rcu+res": (1, 0), "rcu+proj": (0, 1), "rcu+res+proj": (1, 1)}
RCU_FIXED = [(1, 1), (96, 96), (96, 1), (1, 96), (33, 9)]  # (H, W); (33, 9) has the largest accepted LDS footprint
RCU_HOLE = (29, 21)


def rcu_geometries():
    """the fixed members, the smallest accepted map of every class that occurs, the smallest of every ncx"""
    maps = list(RCU_FIXED)
    accepted = sorted(rcu_accepted(), key=lambda hw: (hw[0] * hw[1], hw))
    seen = set()
    for hw in accepted:
        k = rcu_class(*hw)
        if k not in seen:
            seen.add(k)
            maps.append(hw)
    for ncx in range(1, 6):
        maps.append(next(hw for hw in accepted if rcu_geometry(*hw)["ncx"] == ncx))
    return list(dict.fromkeys(maps))


def _rcu_cases():
    out = []
    for H, W in rcu_geometries():
        for mode in RCU_MODES:
            out.append(dict(id=f"rcu-{H}x{W}-{mode}", entry="rcu", kind="random", B=2, H=H, W=W, mode=mode, null=()))
    for mode in RCU_MODES:
        out.append(dict(id=f"rcu-nobias-{mode}", entry="rcu", kind="random", B=2, H=13, W=23, mode=mode, null=("b1", "b2", "bp")))
        out.append(dict(id=f"rcu-nobp-{mode}", entry="rcu", kind="random", B=2, H=13, W=23, mode=mode, null=("bp",)))
    for conv in (1, 2):
        for tap in range(9):
            out.append(dict(id=f"rcu-impulse-conv{conv}-tap{tap}", entry="rcu", kind="impulse", B=2, H=7, W=23, mode="rcu", null=(), conv=conv, tap=tap))
    out.append(dict(id="rcu-large", entry="rcu", kind="large", B=2, H=13, W=23, mode="rcu+res+proj", null=()))
    return out


# ---- bilinear cases -----------------------------------------------------------------------------------------------------------------------

def _bil_cases():
    shapes = [("identity", 7, 9, 7, 9), ("up2", 5, 6, 10, 12), ("half", 12, 10, 6, 5), ("ragged-down", 11, 13, 7, 5), ("h1", 1, 6, 5, 9), ("oh1", 6, 5, 1, 7),
              ("straddle", 3, 20, 4, 43)]  # OW * C / 8 = 43, 129, 344 threads: past one 256-thread block at C = 64
    out = []
    for name, H, W, OH, OW in shapes:
        for C in (8, 24, 64):
            out.append(dict(id=f"bil-{name}-c{C}", entry="bilinear", kind="random", B=2, H=H, W=W, C=C, OH=OH, OW=OW))
    out.append(dict(id="bil-large-c24", entry="bilinear", kind="large", B=2, H=5, W=6, C=24, OH=10, OW=12))
    return out


GROUPS = {"headconv": _head_cases(), "rcu": _rcu_cases(), "bilinear": _bil_cases()}


def group(name):
    return GROUPS[name]


def all_cases():
    return [c for g in GROUPS.values() for c in g]


# ---- the refusals: (fields changed from an accepted base call, message fragment); nothing here is built to fault ---------------------------

HEAD_BASE = dict(B=1, H=17, W=33, hs=10, ws=19, x=1, wfrag=1, bias=1, w3=1, out=1)
HEAD_REFUSALS = ([(dict(**{k: 0}), "null operand") for k in ("x", "wfrag", "bias", "w3", "out")] + [(dict(B=0), "null operand")]
                 + [(dict(H=H, W=W, hs=hs, ws=ws), "outside the kernel's source patch") for _, H, W, hs, ws in HEAD_REFUSED_GEOMETRY]
                 + [(dict(H=1, W=33, hs=1, ws=19), "outside the kernel's source patch"), (dict(hs=1), "outside the kernel's source patch"),
                    (dict(hs=17, ws=33), "outside the kernel's source patch")])
WIDE_REFUSALS = ([(dict(**{k: 0}), "null operand") for k in ("x", "wfrag", "bias", "w3", "out")] + [(dict(B=0), "null operand")]
                 + [(dict(cin=c), f"cin {c} (64 or 128)") for c in (32, 96, 0, 256)]
                 + [(dict(H=H, W=W, hs=hs, ws=ws), "(scale up to 0.58)") for _, H, W, hs, ws in HEAD_REFUSED_GEOMETRY])
RCU_BASE = dict(B=1, H=13, W=23, x=1, w1=1, w2=1, out=1)
RCU_REFUSALS = ([(dict(**{k: 0}), "missing operands") for k in ("x", "w1", "w2", "out")] + [(dict(B=0), "empty batch")]
                + [(dict(H=H, W=W), f"map {W} x {H} is not built") for H, W in (RCU_HOLE, (29, 11), (57, 21), (96, 2), (97, 5), (5, 97), (148, 148), (0, 5))])
BIL_BASE = dict(B=1, H=4, W=4, C=8, OH=8, OW=8, x=1, y=1)
BIL_REFUSALS = [(dict(C=12), "C=12 must be a multiple of 8"), (dict(C=4), "C=4 must be a multiple of 8"), (dict(x=0), "null operand"), (dict(y=0), "null operand"),
                (dict(B=0), "empty extent"), (dict(OH=0), "empty extent"), (dict(W=0), "empty extent"), (dict(C=0), "empty extent"), (dict(OH=65536, OW=1), "do not fit the grid")]


REFUSAL_SCRATCH_BYTES = 16 << 20  # every operand of every table entry fits (148 x 148 x 64 f16 is 2.8 MB): a refusal that regressed stays in bounds


def run_refusals(lib, ptr):
    """every table entry against the library: returns 0 with its message (before any launch: `ptr` is never dereferenced) -> the number run"""
    import ctypes

    from visioncpp_amd import _lib as L

    def p(v):
        return ptr if v else None

    def refused(r, fields, message):
        assert r == 0 and message.encode() in lib.vx_last_error(), (fields, message, lib.vx_last_error())

    n = 0
    for fields, message in HEAD_REFUSALS:
        f = dict(HEAD_BASE, **fields)
        refused(lib.vx_headconv_bil_f16(p(f["x"]), p(f["wfrag"]), p(f["bias"]), p(f["w3"]), 0.0, 1.0, p(f["out"]), f["B"], f["H"], f["W"], f["hs"], f["ws"], None), fields, message)
        n += 1
    for fields, message in WIDE_REFUSALS:
        f = {**HEAD_BASE, "cin": 64, **fields}
        refused(lib.vx_headconv_wide_bil_f16(p(f["x"]), f["cin"], p(f["wfrag"]), p(f["bias"]), p(f["w3"]), 0.0, 1.0, p(f["out"]), f["B"], f["H"], f["W"], f["hs"], f["ws"], None),
                fields, message)
        n += 1
    for fields, message in RCU_REFUSALS:
        f = dict(RCU_BASE, **fields)
        d = L.RcuArgs()
        d.x, d.w1, d.w2, d.out, d.B, d.H, d.W = p(f["x"]), p(f["w1"]), p(f["w2"]), p(f["out"]), f["B"], f["H"], f["W"]
        refused(lib.vx_rcu_fused_f16(ctypes.byref(d), None), fields, message)
        if "H" in fields:  # the message says what is refused
            assert b"512 pixels" in lib.vx_last_error() and b"160 KB" in lib.vx_last_error() and lib.vx_rcu_supported(f["H"], f["W"]) == 0
        n += 1
    for fields, message in BIL_REFUSALS:
        f = dict(BIL_BASE, **fields)
        refused(lib.vx_bilinear_ac_f16(p(f["x"]), p(f["y"]), f["B"], f["H"], f["W"], f["C"], f["OH"], f["OW"], None), fields, message)
        n += 1
    return n


# ---- materialize ------------------------------------------------------------------------------------------------------------------------------

NAN_TAIL = 64  # f16 NaNs behind the source tensor: allocated memory that no accepted call may weigh in


def _f16(a):
    return np.asarray(a).astype(np.float16)


def _with_tail(x):
    return np.concatenate([_f16(x).reshape(-1), np.full(NAN_TAIL, np.nan, np.float16)])


def _materialize_head(c, rng):
    B, H, W, hs, ws, cin, kind = c["B"], c["H"], c["W"], c["hs"], c["ws"], c["cin"], c["kind"]
    a = dict(B=B, H=H, W=W, hs=hs, ws=ws, cin=cin, b3=c.get("b3", 0.05), scale=c.get("scale", 2.5))
    x = rng.standard_normal((B, hs, ws, cin)) * 0.7
    rows = rng.standard_normal((32, 9, cin)) / np.sqrt(9 * cin)
    bias = rng.standard_normal(32) * 0.1
    w3 = rng.standard_normal(32) / 4
    if kind == "impulse":  # one source pixel and channel, one weight: the expected map is that pixel's resized footprint, shifted by the tap
        s, tap = c["slice"], c["tap"]
        _, sy, sx = IMPULSE_AT[c["at"]]
        ch, n = 32 * s + (7 * tap + 3) % 32, (3 * tap + s) % 32
        x = np.zeros_like(x)
        x[B - 1, sy % hs, sx % ws, ch] = 1.5
        rows = np.zeros_like(rows)
        rows[n, tap, ch] = 1.0
        bias, w3 = np.zeros(32), np.full(32, 0.25)
        w3[n] = 1.0
        a.update(b3=0.0, scale=1.0)
    elif kind in ("positive", "negative"):  # no cancellation anywhere: sum |x| |w| |w3| is the sum itself
        x, rows, bias, w3 = np.abs(x), np.abs(rows) * 2.0 / np.sqrt(9 * cin), np.abs(bias), np.abs(w3) / 4
        if kind == "negative":
            # the right half of the source is dim; 24 of 32 channels lie far below zero (their ReLU gives exactly 0 on any correct device), and b3
            # puts the dim half's dot product far below zero too: that region is exactly 0 and compared with allowance 0
            x[:, :, ws // 2:] *= 0.03
            kept = np.arange(32) % 4 == 0
            bright, dim = (float(((rows.sum(axis=(1, 2)) * m + bias) * w3)[kept].sum()) for m in (0.56, 0.56 * 0.03))  # the two halves' dot products, roughly
            bias = np.where(kept, bias, -8.0 * np.sqrt(cin / 32))
            a.update(b3=-float(np.sqrt(bright * dim)))
    elif kind == "large":     # magnitudes of a few hundred; f16 intermediates stay finite (checked against the reference by the CPU test)
        x = x * 400.0
        rows = rows * 3.0
        bias = bias * 100.0
    a.update(x=_with_tail(x), wfrag=R.pack_frag(_f16(rows).reshape(32, -1), cin), bias=bias.astype(np.float32), w3=w3.astype(np.float32), rows=_f16(rows))
    return a


def _materialize_rcu(c, rng):
    B, H, W, kind = c["B"], c["H"], c["W"], c["kind"]
    res, proj = RCU_MODES[c["mode"]]
    x = rng.standard_normal((B, H, W, 64)) * 0.7
    w1, w2 = (rng.standard_normal((64, 9, 64)) / np.sqrt(576) for _ in range(2))
    b = {k: rng.standard_normal(64) * 0.1 for k in ("b1", "b2", "bp")}
    res2 = rng.standard_normal((B, H, W, 64)) * 0.7
    wp = rng.standard_normal((64, 1, 64)) / 8
    if kind == "impulse":  # conv 1: one pixel, one weight of w1, w2 = identity at the centre; conv 2: w1 = identity at the centre, one weight of w2
        tap, ch, n = c["tap"], (5 * c["tap"] + 2) % 64, (11 * c["tap"] + 7) % 64
        x = np.zeros_like(x)
        x[B - 1, H // 2, W // 2, ch] = 1.5
        eye = np.zeros((64, 9, 64))
        eye[np.arange(64), 4, np.arange(64)] = 1.0
        hot = np.zeros((64, 9, 64))
        if c["conv"] == 1:
            hot[n, tap, ch] = 1.0
            w1, w2 = hot, eye
        else:
            hot[n, tap, ch] = 1.0
            w1, w2 = eye, hot
        b = {k: np.zeros(64) for k in b}
    elif kind == "large":
        x, res2 = x * 300.0, res2 * 300.0
        b = {k: v * 100.0 for k, v in b.items()}
    a = dict(B=B, H=H, W=W, x=_with_tail(x), w1=R.pack_rcu(w1), w2=R.pack_rcu(w2), res2=None, wp=None)
    for k in ("b1", "b2", "bp"):
        a[k] = None if (k in c["null"] or (k == "bp" and not proj)) else b[k].astype(np.float32)
    if res:
        a["res2"] = _f16(res2).reshape(-1)
    if proj:
        a["wp"] = R.pack_rcu(wp)
    return a


def _materialize_bil(c, rng):
    B, H, W, C = c["B"], c["H"], c["W"], c["C"]
    x = rng.standard_normal((B, H, W, C)) * (400.0 if c["kind"] == "large" else 0.7)
    return dict(B=B, H=H, W=W, C=C, OH=c["OH"], OW=c["OW"], x=_with_tail(x))


def materialize(c) -> dict:
    rng = np.random.default_rng(zlib.crc32(c["id"].encode()))
    return {"headconv": _materialize_head, "rcu": _materialize_rcu, "bilinear": _materialize_bil}[c["entry"]](c, rng)


def guard_of(c, a) -> int:
    """elements behind the last image: one full tile row of the kernel, and never fewer than 64"""
    th = rcu_geometry(c["H"], c["W"])["TH"] if c["entry"] == "rcu" else None
    return max(R.min_guard(c["entry"], a, th), 64)


def batch_slice(c, a, b) -> dict:
    """the same call on image b alone (B = 1)"""
    out = dict(a, B=1)
    per = {"headconv": lambda: a["hs"] * a["ws"] * a["cin"], "rcu": lambda: a["H"] * a["W"] * 64, "bilinear": lambda: a["H"] * a["W"] * a["C"]}[c["entry"]]()
    out["x"] = np.concatenate([a["x"][b * per:(b + 1) * per], np.full(NAN_TAIL, np.nan, np.float16)])
    if a.get("res2") is not None:
        out["res2"] = a["res2"][b * per:(b + 1) * per]
    return out

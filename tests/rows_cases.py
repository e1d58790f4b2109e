"""The case tables of the row kernels' argument space -- the LayerNorms (vx_layernorm_f32_f16, vx_layernorm_f16, vx_swin_layernorm_f16,
vx_swin_layernorm_strided_f16, vx_swin_merge_layernorm_f16), the window reverse + residual adds (vx_swin_window_reverse_add_f16,
vx_window_reverse_add_f16), vx_dwconv3x3_f16, vx_add_gelu_f16 and vx_add_rows_f16 -- built the same way by the CPU tests that check their
completeness (tests/test_rows_ref_cpu.py) and by the GPU tests that run them (tests/test_gpu_rows_matrix.py). A case is a small dict of data
only; `materialize` turns it into the `args` dict of tests/rows_ref.py: operands drawn once in float64, seeded by the case id, and rounded to
the type the kernel reads. The launchers' `if` chains are restated here from csrc/kernels_misc.hip, kernels_tinyvit.hip and kernels_swin.hip.

Data kinds of the LayerNorms: `normal` (sigma 2, mean 0.3), `offset` (mean 40, sigma 0.5), `tiny` (sigma 2e-3: eps decides the result),
`constant` (every element of a row equal, a constant of its own per row), `outlier` (one element of +-60000 per row, the rest standard
normal), `scales` (row r times 2^((r mod 17) - 8): rows that share a wave differ by orders of magnitude). Gains hold exact zeros and negative
values; eps alternates between 1e-5 and 1e-6 and every `tiny` case exists with both."""
from __future__ import annotations

import zlib

import numpy as np

import rows_ref as R

KINDS = ("normal", "offset", "tiny", "constant", "outlier", "scales")
EPS = (1e-5, 1e-6)

# ---- the launchers, restated ----------------------------------------------------------------------------------------------------------------

LN32_VECTOR = {128: "vec1", 384: "vec3", 768: "vec6", 1024: "vec8"}  # layernorm_vec_kernel<C / 128>


def ln32_class(C):
    """vx_layernorm_f32_f16: one of the four vector kernels, or the generic one with fewer elements than lanes, as many, or more"""
    return LN32_VECTOR.get(C) or ("generic", "<64" if C < 64 else "=64" if C == 64 else ">64")


LN32_CLASSES = set(LN32_VECTOR.values()) | {("generic", s) for s in ("<64", "=64", ">64")}


def _edge(C, lo, hi):
    return "lo" if C == lo else "hi" if C == hi else "mid"


def _chain(C, bounds):
    """the class of C in an `if (C <= b0) .. else if (C <= b1) ..` chain over multiples of 8: (index of the branch, where C stands in it: `lo`
    one step past the boundary below, `hi` at the branch's own limit, `mid` between them)"""
    lo = 8
    for i, hi in enumerate(bounds):
        if C <= hi:
            return i, _edge(C, lo, hi)
        lo = hi + 8
    raise ValueError(C)


TV_LN_BOUNDS = (128, 256, 512, 1024)             # tv_layernorm_kernel<16 | 32 | 64>, tv_layernorm_wide_kernel<2>
SWIN_LN_BOUNDS = (128, 256, 512, 1024, 2048)     # swin_ln_rows_kernel<16,1 | 32,1 | 64,1 | 64,2 | 64,4>
SWIN_MERGE_BOUNDS = (128, 256, 512, 1024, 2048, 4096)  # swin_merge_ln_kernel<..., 64,8> on 4 C


def tv_ln_class(C):
    return _chain(C, TV_LN_BOUNDS)


def swin_ln_class(C):
    return _chain(C, SWIN_LN_BOUNDS)


def swin_merge_class(C):
    i, edge = _chain(4 * C, SWIN_MERGE_BOUNDS)
    if edge == "mid" and 4 * C == (SWIN_MERGE_BOUNDS[i - 1] if i else 0) + 32:
        edge = "lo"  # 4 C moves in steps of 32: the first width behind a boundary
    return i, edge


def chain_classes(bounds):
    return {(i, e) for i in range(len(bounds)) for e in ("lo", "hi")}


def dwconv_blocks(c) -> int:
    """vx_dwconv3x3_f16's own formula: one thread = P output pixels of one row x 8 channels, 256 threads per block"""
    OH, OW = R.dwconv_extent(c["H"], c["W"], c["stride"])
    P = 8 if c["stride"] == 1 else 4
    n = c["B"] * OH * ((OW + P - 1) // P) * (c["C"] // 8)
    return (n + 255) // 256


def dwconv_block_order(nwg):
    """tv_dwconv3x3_kernel's XCD-aware order: hardware block b computes block order[b] of the row-major sequence"""
    b = np.arange(nwg)
    q, rem, xcd = nwg >> 3, nwg & 7, b & 7
    return np.where(xcd < rem, xcd * (q + 1), rem * (q + 1) + (xcd - rem) * q) + (b >> 3)


# ---- the tables ---------------------------------------------------------------------------------------------------------------------------------

LN32_C = (128, 384, 768, 1024, 1, 8, 63, 64, 65, 200, 1536)
LN32_M = (1, 4, 5, 131)
TV_LN_C = (8, 128, 136, 256, 264, 512, 520, 768, 1024)
TV_WINDOWS = ((10, 4), (9, 4), (7, 7))  # (res, ws)
SWIN_LN_C = (8, 128, 136, 256, 264, 512, 520, 1024, 1032, 2048)
SWIN_MAPS = ((9, 8), (5, 13), (7, 7), (14, 21))  # (H, W)
SWIN_WINDOWS = ((7, 0), (7, 3), (4, 1), (4, 3))  # (ws, shift)
SWIN_MERGE_C = (8, 32, 40, 64, 72, 128, 136, 256, 264, 512, 520, 1024)
SWIN_MERGE_MAPS = ((2, 2), (4, 6), (6, 10))
PLAIN_ROWS = 37  # 2 blocks and 5 rows of 16, 4 blocks and 5 rows of 8, 9 blocks and 1 row of 4; more than 17 rows for `scales`
REVERSE_C = (8, 96)
DW_W = {1: (1, 7, 8, 9, 17), 2: (1, 2, 7, 8, 9)}
DW_H = (1, 2, 5)
DW_C = (8, 24, 160)
DW_BLOCK_SHAPES = [  # (stride, B, H, W, C): block counts 7, 8, 9, 19 at stride 1 and 7, 9 at stride 2
    (1, 2, 5, 57, 160), (1, 2, 5, 79, 160), (1, 2, 5, 81, 160), (1, 3, 7, 81, 160), (2, 2, 9, 57, 160), (2, 2, 9, 81, 160)]
ADD_N = (8, 8 * 257, 8 * 1000)
ADD_PERIODS = {8: (8, 16), 8 * 257: (8 * 257, 8, 16), 8 * 1000: (8 * 1000, 800, 1536)}  # equal to n, dividing n, not dividing n
GELU_PLANTS = (11.0, -11.0, 40.0, -40.0, 60000.0, -60000.0)


def _smallest(bounds):
    return [8] + [b + 8 for b in bounds[:-1]]


def _eps(i):
    return EPS[i & 1]


def _ln32_cases():
    out = []
    for C in LN32_C:
        for M in LN32_M:
            out.append(dict(id=f"ln32-c{C}-m{M}", entry="ln32", kind="normal", C=C, M=M, eps=_eps(len(out))))
    for C in (128, 384, 768, 1024, 1, 8, 64, 65):  # the smallest C of every class
        for kind in KINDS[1:]:
            for eps in (EPS if kind == "tiny" else (_eps(len(out)),)):
                out.append(dict(id=f"ln32-c{C}-{kind}-eps{eps:g}", entry="ln32", kind=kind, C=C, M=PLAIN_ROWS, eps=eps))
    out.append(dict(id="ln32-c384-zero-bias", entry="ln32", kind="normal", C=384, M=5, eps=1e-6, zero_bias=True))
    out.append(dict(id="ln32-c200-zero-bias", entry="ln32", kind="normal", C=200, M=5, eps=1e-5, zero_bias=True))
    return out


def _tv_ln(cid, C, layout, out_f32, kind="normal", eps=1e-5, **more):
    c = dict(id=cid, entry="tv_ln", kind=kind, C=C, out_f32=out_f32, eps=eps, res=0, ws=0, B=1, **more)
    if layout == "rows":
        c["rows_out"] = PLAIN_ROWS
    elif layout == "row":
        c["rows_out"] = 1
    else:
        res, ws = layout
        nw = -(-res // ws)
        c.update(res=res, ws=ws, B=2, rows_out=2 * nw * nw * ws * ws)
    return c


def _tv_ln_cases():
    out = []
    for C in TV_LN_C:
        for layout in ("rows",) + TV_WINDOWS:
            for out_f32 in (0, 1):
                tag = "rows" if layout == "rows" else f"res{layout[0]}ws{layout[1]}"
                out.append(_tv_ln(f"tvln-c{C}-{tag}-{'f32' if out_f32 else 'f16'}", C, layout, out_f32, eps=_eps(len(out))))
        out.append(_tv_ln(f"tvln-c{C}-onerow", C, "row", 0, eps=_eps(len(out))))
    for C in _smallest(TV_LN_BOUNDS):
        for kind in KINDS[1:]:
            for eps in (EPS if kind == "tiny" else (_eps(len(out)),)):
                out.append(_tv_ln(f"tvln-c{C}-{kind}-eps{eps:g}-res9ws4-f16", C, (9, 4), 0, kind, eps))
                out.append(_tv_ln(f"tvln-c{C}-{kind}-eps{eps:g}-rows-f32", C, "rows", 1, kind, eps))
    out.append(_tv_ln("tvln-c136-zero-bias", 136, (9, 4), 0, zero_bias=True))
    return out


def _swin_ln(cid, C, layout, out_f32=0, kind="normal", eps=1e-5, **more):
    c = dict(id=cid, entry="swin_ln", kind=kind, C=C, out_f32=out_f32, eps=eps, H=0, W=0, ws=0, shift=0, B=1, rows_out=PLAIN_ROWS, **more)
    if layout != "rows":
        (H, W), (ws, shift) = layout
        c.update(H=H, W=W, ws=ws, shift=shift, B=2, rows_out=2 * -(-H // ws) * -(-W // ws) * ws * ws)
    return c


def _swin_ln_cases():
    out = []
    for i, C in enumerate(SWIN_LN_C):
        for out_f32 in (0, 1):
            out.append(_swin_ln(f"swinln-c{C}-rows-{'f32' if out_f32 else 'f16'}", C, "rows", out_f32, eps=_eps(len(out))))
        for j, hw in enumerate(SWIN_MAPS):  # every map with every window at C = 8 and 136; at the other widths every map with one window each
            for k, win in enumerate(SWIN_WINDOWS):
                if C in (8, 136) or k == (i + j) % 4:
                    out.append(_swin_ln(f"swinln-c{C}-{hw[0]}x{hw[1]}-ws{win[0]}s{win[1]}", C, (hw, win), eps=_eps(len(out))))
    for C in _smallest(SWIN_LN_BOUNDS):
        for kind in KINDS[1:]:
            for eps in (EPS if kind == "tiny" else (_eps(len(out)),)):
                out.append(_swin_ln(f"swinln-c{C}-{kind}-eps{eps:g}-5x13-ws4s1", C, ((5, 13), (4, 1)), 0, kind, eps))
                out.append(_swin_ln(f"swinln-c{C}-{kind}-eps{eps:g}-rows-f32", C, "rows", 1, kind, eps))
    out.append(_swin_ln("swinln-c136-zero-bias", 136, ((5, 13), (4, 3)), zero_bias=True))
    return out


def _swin_ln_strided_cases():
    out = []

    def one(cid, C, ldy, out_f32, kind="normal", eps=1e-5, **more):
        return dict(id=cid, entry="swin_ln_strided", kind=kind, C=C, ldy=ldy, out_f32=out_f32, eps=eps, rows_out=PLAIN_ROWS, **more)

    for C in SWIN_LN_C:
        for ldy in dict.fromkeys((C + 8, 2 * C)):  # (one stride at C = 8)
            for out_f32 in (0, 1):
                out.append(one(f"swinlds-c{C}-ld{ldy}-{'f32' if out_f32 else 'f16'}", C, ldy, out_f32, eps=_eps(len(out))))
    for C in _smallest(SWIN_LN_BOUNDS):
        for kind in KINDS[1:]:
            for eps in (EPS if kind == "tiny" else (_eps(len(out)),)):
                out.append(one(f"swinlds-c{C}-{kind}-eps{eps:g}-ld{C + 8}-f16", C, C + 8, 0, kind, eps))
    out.append(one("swinlds-c264-zero-bias", 264, 272, 0, zero_bias=True))
    out.append(one("swinlds-c8-ld0", 8, 0, 0))  # 0 = C: rows back to back
    return out


def _swin_merge_cases():
    out = []

    def one(cid, C, hw, kind="normal", eps=1e-5, **more):
        return dict(id=cid, entry="swin_merge", kind=kind, C=C, B=2, H=hw[0], W=hw[1], eps=eps, **more)

    for C in SWIN_MERGE_C:
        for hw in SWIN_MERGE_MAPS:
            out.append(one(f"merge-c{C}-{hw[0]}x{hw[1]}", C, hw, eps=_eps(len(out))))
    for C in (8, 40, 72, 136, 264, 520):  # 4 C one step behind every boundary
        for kind in KINDS[1:]:
            for eps in (EPS if kind == "tiny" else (_eps(len(out)),)):
                out.append(one(f"merge-c{C}-{kind}-eps{eps:g}-6x10", C, (6, 10), kind, eps))
    out.append(one("merge-c72-zero-bias", 72, (4, 6), zero_bias=True))
    return out


def _reverse_cases():
    swin = [dict(id=f"swinrev-c{C}-{H}x{W}-ws{ws}s{shift}", entry="swin_reverse", kind="normal", C=C, B=2, H=H, W=W, ws=ws, shift=shift)
            for C in REVERSE_C for H, W in SWIN_MAPS for ws, shift in SWIN_WINDOWS]
    tv = [dict(id=f"tvrev-c{C}-res{res}ws{ws}", entry="tv_reverse", kind="normal", C=C, B=2, res=res, ws=ws) for C in REVERSE_C for res, ws in TV_WINDOWS]
    return swin, tv


def _dwconv_cases():
    out = []
    for stride in (1, 2):
        for W in DW_W[stride]:
            for H in DW_H:
                for C in DW_C:
                    for gelu in (0, 1):
                        out.append(dict(id=f"dw-s{stride}-{H}x{W}-c{C}" + ("-gelu" if gelu else ""), entry="dwconv", kind="normal", B=2, H=H, W=W, C=C, stride=stride, gelu=gelu))
    for i, (stride, Bn, H, W, C) in enumerate(DW_BLOCK_SHAPES):
        out.append(dict(id=f"dw-s{stride}-b{Bn}-{H}x{W}-c{C}-blocks", entry="dwconv", kind="normal", B=Bn, H=H, W=W, C=C, stride=stride, gelu=i & 1))
    for stride in (1, 2):
        for gelu in (0, 1):
            out.append(dict(id=f"dw-s{stride}-5x9-c24-huge" + ("-gelu" if gelu else ""), entry="dwconv", kind="huge", B=2, H=5, W=9, C=24, stride=stride, gelu=gelu))
    return out


def _add_cases():
    g = [dict(id=f"addgelu-n{n}" + ("" if b else "-nob"), entry="add_gelu", kind="normal", n=n, b=b) for n in ADD_N for b in (1, 0)]
    g += [dict(id="addgelu-huge" + ("" if b else "-nob"), entry="add_gelu", kind="huge", n=8 * 257, b=b) for b in (1, 0)]
    r = [dict(id=f"addrows-n{n}-p{p}-{'f32' if f32 else 'f16'}", entry="add_rows", kind="normal", n=n, period=p, a_is_f32=f32) for n in ADD_N for p in ADD_PERIODS[n] for f32 in (0, 1)]
    r.append(dict(id="addrows-inexact-f32", entry="add_rows", kind="inexact", n=8 * 257, period=16, a_is_f32=1))
    return g, r


_SWIN_REV, _TV_REV = _reverse_cases()
_ADD_GELU, _ADD_ROWS = _add_cases()
GROUPS = {"ln32": _ln32_cases(), "tv_ln": _tv_ln_cases(), "swin_ln": _swin_ln_cases(), "swin_ln_strided": _swin_ln_strided_cases(), "swin_merge": _swin_merge_cases(),
          "swin_reverse": _SWIN_REV, "tv_reverse": _TV_REV, "dwconv": _dwconv_cases(), "add_gelu": _ADD_GELU, "add_rows": _ADD_ROWS}
assert len({c["id"] for g in GROUPS.values() for c in g}) == sum(len(g) for g in GROUPS.values())
assert all(c["entry"] == name for name, g in GROUPS.items() for c in g)


def group(name):
    return GROUPS[name]


def all_cases():
    return [c for g in GROUPS.values() for c in g]


def case(cid):
    return next(c for c in all_cases() if c["id"] == cid)


# ---- materialize ------------------------------------------------------------------------------------------------------------------------------

def rows_data(kind, rows, C, rng):
    """[rows, C] float64 of one data kind"""
    z = rng.standard_normal((rows, C))
    if kind == "normal":
        return 0.3 + 2.0 * z
    if kind == "offset":
        return 40.0 + 0.5 * z
    if kind == "tiny":
        return 2e-3 * z
    if kind == "constant":
        return np.broadcast_to(rng.uniform(-8.0, 8.0, (rows, 1)), (rows, C)).copy()
    if kind == "outlier":
        z[np.arange(rows), rng.integers(0, C, rows)] = 60000.0 * rng.choice([-1.0, 1.0], rows)
        return z
    assert kind == "scales"
    return (0.3 + 2.0 * z) * 2.0 ** ((np.arange(rows) % 17) - 8)[:, None]


def gain_bias(width, rng, zero_bias=False):
    """f32 gain with exact zeros (every 7th) and negative values (every 5th from 3), f32 bias"""
    w = 1.0 + 0.5 * rng.standard_normal(width)
    w[3::5] = -np.abs(w[3::5])
    w[::7] = 0.0
    b = np.zeros(width) if zero_bias else 0.2 * rng.standard_normal(width)
    return w.astype(np.float32), b.astype(np.float32)


def _materialize_ln(c, rng):
    entry, C = c["entry"], c["C"]
    a = {k: v for k, v in c.items() if k not in ("id", "entry", "kind", "zero_bias")}
    if entry == "swin_merge":
        rows_in, width = c["B"] * c["H"] * c["W"], 4 * C
    elif entry == "ln32":
        rows_in, width = c["M"], C
    elif c.get("ws"):
        rows_in, width = (c["B"] * c["res"] ** 2 if entry == "tv_ln" else c["B"] * c["H"] * c["W"]), C
    else:
        rows_in, width = c["rows_out"], C
    if entry == "swin_merge":  # the data kind describes the rows the LayerNorm sees: drawn as merged rows of 4 C, scattered to their four pixels
        merged = rows_data(c["kind"], rows_in // 4, width, rng)
        x = np.empty((rows_in, C))
        x[R.merge_gather(c["B"], c["H"], c["W"])] = merged.reshape(-1, 4, C)
    else:
        x = rows_data(c["kind"], rows_in, C, rng)
    a["x"] = x.astype(np.float32) if entry == "ln32" else x.astype(np.float16)
    a["w"], a["b"] = gain_bias(width, rng, c.get("zero_bias", False))
    return a


def _materialize_reverse(c, rng):
    C = c["C"]
    H, W, shift = (c["res"], c["res"], 0) if c["entry"] == "tv_reverse" else (c["H"], c["W"], c["shift"])
    src = R.partition_rows(c["B"], H, W, c["ws"], shift)
    a_rows = (0.3 + 2.0 * rng.standard_normal((src.size, C))).astype(np.float16)
    a_rows[src < 0] = np.nan  # the pad rows of the window buffer are not the call's to read
    x = (0.3 + 2.0 * rng.standard_normal((c["B"] * H * W, C))).astype(np.float16)
    return dict({k: v for k, v in c.items() if k not in ("id", "entry", "kind")}, a=a_rows, x=x)


def _huge(shape, rng):
    """magnitudes in the upper binades of f16 with GELU_PLANTS among them, each below the f16 maximum"""
    v = rng.uniform(30000.0, 60000.0, shape) * rng.choice([-1.0, 1.0], shape)
    flat = v.reshape(-1)
    at = rng.permutation(flat.size)[:len(GELU_PLANTS)]
    flat[at] = GELU_PLANTS
    return v, at


def _materialize_dwconv(c, rng):
    Bn, H, W, C = c["B"], c["H"], c["W"], c["C"]
    a = {k: c[k] for k in ("B", "H", "W", "C", "stride", "gelu")}
    if c["kind"] == "huge":  # the centre tap alone, no bias: every sum IS an input value (of the pixels the stride visits), so no sum overflows f16
        x, _ = _huge((Bn, H, W, C), rng)
        x.reshape(Bn, H, W, C)[0, 0, 0, :len(GELU_PLANTS)] = GELU_PLANTS  # pixel (0, 0) is an output centre at either stride
        w = np.zeros((9, C))
        w[4] = 1.0
        b = np.zeros(C)
    else:
        x = 0.3 + 2.0 * rng.standard_normal((Bn, H, W, C))
        w = rng.standard_normal((9, C)) / 3.0
        b = 0.2 * rng.standard_normal(C)
    a.update(x=x.astype(np.float16), w=w.astype(np.float16), bias=b.astype(np.float32))
    return a


def _materialize_add_gelu(c, rng):
    n = c["n"]
    if c["kind"] == "huge":
        a, at = _huge(n, rng)
        b = np.sign(a) * rng.uniform(0.0, 4000.0, n)  # same sign: |a + b| stays below 64000
        b[at] = 0.0
    else:
        a, b = 2.0 * rng.standard_normal(n), 2.0 * rng.standard_normal(n)
    return dict(n=n, a=a.astype(np.float16), b=b.astype(np.float16) if c["b"] else None)


def _materialize_add_rows(c, rng):
    n, period = c["n"], c["period"]
    a, b = 0.3 + 2.0 * rng.standard_normal(n), 2.0 * rng.standard_normal(period)
    if c["kind"] == "inexact":  # an f32 of 16 .. 2048 with all 24 bits in use (ulp 2^-19 and more) plus an f16 whose last bit is 2^-22: the f32 sum rounds
        a = (1.0 + rng.integers(0, 2 ** 23, n) * 2.0 ** -23) * 2.0 ** rng.integers(4, 11, n) * rng.choice([-1.0, 1.0], n)
        b = (1.0 + rng.integers(0, 2 ** 10, period) * 2.0 ** -10) * 2.0 ** -12
    return dict(n=n, period=period, a_is_f32=c["a_is_f32"], a=a.astype(np.float32) if c["a_is_f32"] else a.astype(np.float16), b=b.astype(np.float16))


def materialize(c) -> dict:
    rng = np.random.default_rng(zlib.crc32(c["id"].encode()))
    e = c["entry"]
    if e in R.LAYER_NORMS:
        return _materialize_ln(c, rng)
    return {"swin_reverse": _materialize_reverse, "tv_reverse": _materialize_reverse, "dwconv": _materialize_dwconv, "add_gelu": _materialize_add_gelu,
            "add_rows": _materialize_add_rows}[e](c, rng)


def guard_of(c, a) -> int:
    return R.min_guard(c["entry"], a)


# ---- the refusals: (fields changed from an accepted base call, message fragment); nothing here is built to fault ---------------------------
# Pointer fields hold 1 (the scratch buffer) or 0 (NULL). Every base call, and every call of the tables should its refusal regress, stays
# inside the scratch buffer.

_NULL = "null operand"
LN32_BASE = dict(x=1, w=1, b=1, y=1, M=4, C=64)
LN32_REFUSALS = [(dict(**{k: 0}), _NULL) for k in ("x", "w", "b", "y")] + [(dict(M=0), "empty problem"), (dict(C=0), "empty problem"), (dict(M=-1), "empty problem")]
TV_LN_BASE = dict(x=1, w=1, b=1, y=1, rows_out=4, C=64, res=0, ws=0, out_f32=0)
TV_LN_REFUSALS = ([(dict(**{k: 0}), "vx_layernorm_f16: bad operands") for k in ("x", "w", "b", "y")]
                  + [(dict(C=12), "bad operands (C = 12"), (dict(C=4), "bad operands (C = 4"), (dict(C=1032), "bad operands (C = 1032"), (dict(C=0), "bad operands (C = 0"),
                     (dict(rows_out=0), "bad operands"), (dict(res=10, ws=4, rows_out=100), "rows do not form whole images of 3 x 3 windows"),
                     (dict(res=7, ws=7, rows_out=48), "rows do not form whole images of 1 x 1 windows")])
SWIN_LN_BASE = dict(x=1, w=1, b=1, y=1, rows_out=64, C=8, H=5, W=5, ws=4, shift=1, out_f32=0)
_SWIN_BAD = "vx_swin_layernorm_f16: bad operands"
SWIN_LN_REFUSALS = ([(dict(**{k: 0}), _SWIN_BAD) for k in ("x", "w", "b", "y")]
                    + [(dict(C=12), _SWIN_BAD + " (C = 12"), (dict(C=2056), _SWIN_BAD + " (C = 2056"), (dict(C=0), _SWIN_BAD), (dict(rows_out=0), _SWIN_BAD),
                       (dict(rows_out=60), "rows do not form whole images of 5x5 maps in windows of 4"), (dict(H=9, rows_out=64), "rows do not form whole images"),
                       (dict(shift=4), "bad window arguments"), (dict(shift=7), "bad window arguments"), (dict(shift=-1), "bad window arguments"),
                       (dict(out_f32=1), "bad window arguments"), (dict(H=0), "bad window arguments"), (dict(W=0), "bad window arguments")])
SWIN_LN_STRIDED_BASE = dict(x=1, w=1, b=1, y=1, rows=4, C=64, ldy=72, out_f32=0)
SWIN_LN_STRIDED_REFUSALS = [(dict(ldy=56), "row stride 56 for 64 channels"), (dict(ldy=68), "row stride 68 for 64 channels"), (dict(ldy=-8), "row stride -8"),
                            (dict(C=12, ldy=16), _SWIN_BAD + " (C = 12"), (dict(C=2056, ldy=2056), _SWIN_BAD + " (C = 2056"), (dict(y=0), _SWIN_BAD)]
SWIN_MERGE_BASE = dict(x=1, w=1, b=1, y=1, B=1, H=4, W=6, C=8)
_MERGE_BAD = "vx_swin_merge_layernorm_f16: bad operands"
SWIN_MERGE_REFUSALS = ([(dict(**{k: 0}), _MERGE_BAD) for k in ("x", "w", "b", "y")]
                       + [(dict(C=12), _MERGE_BAD + " (C = 12"), (dict(C=1032), _MERGE_BAD + " (C = 1032"), (dict(C=0), _MERGE_BAD), (dict(B=0), _MERGE_BAD),
                          (dict(H=3), "even spatial dimensions, got 6x3"), (dict(W=5), "even spatial dimensions, got 5x4"), (dict(H=0), "even spatial dimensions")])
SWIN_REVERSE_BASE = dict(a=1, x=1, y=1, B=1, H=5, W=5, C=8, ws=4, shift=1)
_REV_BAD = "vx_swin_window_reverse_add_f16: bad operands"
SWIN_REVERSE_REFUSALS = ([(dict(**{k: 0}), _REV_BAD) for k in ("a", "x", "y")]
                         + [(f, _REV_BAD) for f in (dict(C=12), dict(C=0), dict(shift=4), dict(shift=-1), dict(ws=0), dict(B=0), dict(H=0))])
TV_REVERSE_BASE = dict(a=1, x=1, y=1, B=1, res=5, ws=4, C=8)
_TVREV_BAD = "vx_window_reverse_add_f16: bad operands"
TV_REVERSE_REFUSALS = [(dict(**{k: 0}), _TVREV_BAD) for k in ("a", "x", "y")] + [(f, _TVREV_BAD) for f in (dict(C=12), dict(C=0), dict(ws=0), dict(res=0), dict(B=0))]
DWCONV_BASE = dict(x=1, w=1, bias=1, y=1, B=1, H=3, W=3, C=8, stride=1, gelu=0)
DWCONV_REFUSALS = ([(dict(**{k: 0}), "vx_dwconv3x3_f16: bad operands") for k in ("x", "w", "bias", "y")]
                   + [(dict(stride=3), "(C = 8, stride = 3)"), (dict(stride=0), "(C = 8, stride = 0)"), (dict(C=12), "(C = 12, stride = 1)"), (dict(C=0), "(C = 0, stride = 1)"),
                      (dict(C=0, stride=2), "(C = 0, stride = 2)"), (dict(H=0), "vx_dwconv3x3_f16: bad operands"), (dict(B=0), "vx_dwconv3x3_f16: bad operands")])
ADD_GELU_BASE = dict(a=1, b=1, y=1, n=64)
ADD_GELU_REFUSALS = [(f, "vx_add_gelu_f16: n must be a positive multiple of 8") for f in (dict(n=12), dict(n=0), dict(n=-8), dict(a=0), dict(y=0))]
ADD_ROWS_BASE = dict(a=1, a_is_f32=0, b=1, period=16, y=1, n=64)
ADD_ROWS_REFUSALS = [(f, "vx_add_rows_f16: n and the period must be positive multiples of 8")
                     for f in (dict(n=12), dict(n=0), dict(period=12), dict(period=0), dict(period=-8), dict(a=0), dict(b=0), dict(y=0), dict(n=12, a_is_f32=1))]
REFUSAL_TABLES = {"ln32": LN32_REFUSALS, "tv_ln": TV_LN_REFUSALS, "swin_ln": SWIN_LN_REFUSALS, "swin_ln_strided": SWIN_LN_STRIDED_REFUSALS, "swin_merge": SWIN_MERGE_REFUSALS,
                  "swin_reverse": SWIN_REVERSE_REFUSALS, "tv_reverse": TV_REVERSE_REFUSALS, "dwconv": DWCONV_REFUSALS, "add_gelu": ADD_GELU_REFUSALS, "add_rows": ADD_ROWS_REFUSALS}
REFUSAL_BASES = {"ln32": LN32_BASE, "tv_ln": TV_LN_BASE, "swin_ln": SWIN_LN_BASE, "swin_ln_strided": SWIN_LN_STRIDED_BASE, "swin_merge": SWIN_MERGE_BASE,
                 "swin_reverse": SWIN_REVERSE_BASE, "tv_reverse": TV_REVERSE_BASE, "dwconv": DWCONV_BASE, "add_gelu": ADD_GELU_BASE, "add_rows": ADD_ROWS_BASE}
N_REFUSALS = sum(len(t) for t in REFUSAL_TABLES.values())

REFUSAL_SCRATCH_BYTES = 1 << 20


def call(lib, entry, f, p, eps=1e-5):
    """one call of launcher `entry` with the fields f; p(field) turns a pointer field into an address or NULL"""
    if entry == "ln32":
        return lib.vx_layernorm_f32_f16(p(f["x"]), p(f["w"]), p(f["b"]), p(f["y"]), f["M"], f["C"], eps, None)
    if entry == "tv_ln":
        return lib.vx_layernorm_f16(p(f["x"]), p(f["w"]), p(f["b"]), p(f["y"]), f["rows_out"], f["C"], eps, f["res"], f["ws"], f["out_f32"], None)
    if entry == "swin_ln":
        return lib.vx_swin_layernorm_f16(p(f["x"]), p(f["w"]), p(f["b"]), p(f["y"]), f["rows_out"], f["C"], eps, f["H"], f["W"], f["ws"], f["shift"], f["out_f32"], None)
    if entry == "swin_ln_strided":
        return lib.vx_swin_layernorm_strided_f16(p(f["x"]), p(f["w"]), p(f["b"]), p(f["y"]), f["rows"], f["C"], eps, f["ldy"], f["out_f32"], None)
    if entry == "swin_merge":
        return lib.vx_swin_merge_layernorm_f16(p(f["x"]), p(f["w"]), p(f["b"]), p(f["y"]), f["B"], f["H"], f["W"], f["C"], eps, None)
    if entry == "swin_reverse":
        return lib.vx_swin_window_reverse_add_f16(p(f["a"]), p(f["x"]), p(f["y"]), f["B"], f["H"], f["W"], f["C"], f["ws"], f["shift"], None)
    if entry == "tv_reverse":
        return lib.vx_window_reverse_add_f16(p(f["a"]), p(f["x"]), p(f["y"]), f["B"], f["res"], f["ws"], f["C"], None)
    if entry == "dwconv":
        return lib.vx_dwconv3x3_f16(p(f["x"]), p(f["w"]), p(f["bias"]), p(f["y"]), f["B"], f["H"], f["W"], f["C"], f["stride"], f["gelu"], None)
    if entry == "add_gelu":
        return lib.vx_add_gelu_f16(p(f["a"]), p(f["b"]), p(f["y"]), f["n"], None)
    assert entry == "add_rows"
    return lib.vx_add_rows_f16(p(f["a"]), f["a_is_f32"], p(f["b"]), f["period"], p(f["y"]), f["n"], None)


def run_refusals(lib, ptr, seen=None):
    """every table entry against the library: returns 0 with its message (before any launch: `ptr` is never dereferenced) -> the number run;
    `seen` collects (entry, message)"""
    n = 0
    for entry, table in REFUSAL_TABLES.items():
        for fields, message in table:
            f = dict(REFUSAL_BASES[entry], **fields)
            r = call(lib, entry, f, lambda flag: ptr if flag else None)
            assert r == 0 and message.encode() in lib.vx_last_error(), (entry, fields, message, lib.vx_last_error())
            if seen is not None:
                seen.append((entry, lib.vx_last_error().decode()))
            n += 1
    return n

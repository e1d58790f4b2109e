"""The case tables of the image entry and exit kernels' argument space -- vx_preprocess_patches, vx_preprocess_f32, vx_write_cls_rows,
vx_head_out_f32, vx_minmax_normalize, vx_f32_to_u8, vx_tv_preprocess, vx_bf_preprocess_half, vx_bf_patches, vx_sam_interpolate -- built the
same way by the CPU tests that check their completeness (tests/test_pixel_ref_cpu.py) and by the GPU tests that run them
(tests/test_gpu_pixel_matrix.py). A case is a small dict of data only; `materialize` turns it into the `args` dict of tests/pixel_ref.py,
seeded by the case id. The launchers' `if` chains are restated here from csrc/kernels_misc.hip, kernels_tinyvit.hip and kernels_birefnet.hip.
The shapes are the smallest that reach each path; the three grid-stride kernels each get one case of 4096 x 256 + 3 elements or more.

Images: `ramp` (pixel i of image b holds byte (37 i + 85 c + 11 b) mod 256 in channel c: every channel of an image of 256 pixels or more holds
all 256 byte values) and `random`. vx_minmax_normalize takes FINITE input (its contract); its data kinds: `mixed` (both signs), `negative`,
`zeros` (non-negative, the minimum a -0.0 next to a +0.0), `subnormal` (every value an f32 subnormal, both signs), `huge` (magnitudes near
1e30), `const0` and `const` (constant images), `below` / `above` (max - min one f32 step below 1e-5f, and 1e-5f itself). The extremes of
`mixed`, `negative` and `huge` are planted: at the first element, the last element of the 16-byte body, the last element (the tail) or the
middle, rotating with the image and the case."""
from __future__ import annotations

import ctypes
import zlib

import numpy as np

import pixel_ref as R

F32 = np.float32

# ---- the launchers, restated -------------------------------------------------------------------------------------------------------------------

HEAD_OUT_WIDTHS = (8, 16, 32, 64)                  # head_out_kernel<C>; any other C is refused
STRIDE_LOOP_N = R.GRID_CAP * R.BLOCK + 3           # the smallest count past one pass of a full grid, plus a partial block's worth
MINMAX_CAP = 64                                    # grid_stride_blocks(n, 64): blocks per image of normalize_kernel


def patches_instance(ps):
    """vx_preprocess_patches: preprocess_patches_kernel<14> or the runtime-patch-size instance <0>"""
    return "ps14" if ps == 14 else "runtime"


def stride_blocks(n, cap=R.GRID_CAP):
    """vx_common.h's grid_stride_blocks(n, cap): at least one block, at most cap blocks of 256"""
    return max(1, min(-(-n // R.BLOCK), cap))


def loops(n, cap=R.GRID_CAP):
    return n > stride_blocks(n, cap) * R.BLOCK


def minmax_class(B):
    """blocks per image of the reduction before the grid-stride cap"""
    return 16 if B >= 16 else 32 if B >= 4 else 64


def minmax_grids(B, n):
    """(blocks per image of minmax_kernel, of normalize_kernel)"""
    gx = stride_blocks(n, MINMAX_CAP)
    return min(minmax_class(B), gx), gx


def image_aligned(b, n):
    """minmax_kernel takes 16-byte loads when the image starts on a 16-byte boundary (the buffer itself does)"""
    return (b * n) % 4 == 0


def bf_patches_path(CP):
    """bf_patches_kernel: 16-byte stores when every pixel's row is 16-byte aligned, else element by element (a partial last chunk, and full
    chunks before it where CP > 8)"""
    return "vector" if CP % 8 == 0 else "scalar-partial" if CP < 8 else "scalar-full+partial"


# ---- the tables -----------------------------------------------------------------------------------------------------------------------------------

PATCH_SIZES = ((14, 592), (16, 768), (8, 192), (8, 200), (3, 32), (1, 8))  # (ps, Kp): 16 without padding, 8 with and without
PATCH_GRIDS = ((1, 1), (2, 3), (3, 2))                                      # (ph, pw)
PATCH_BIG_GRIDS = {3: (6, 6), 1: (16, 17)}                                  # 256 pixels or more for the patch sizes whose grids above hold fewer
NORMS = ("imagenet", "identity")
PRE32_SHAPES = ((1, 1, 1), (2, 3, 5), (1, 600, 600))
CLS_B, CLS_T, CLS_C = (1, 3), (1, 2, 5), (1, 96, 128, 130, 384, 1024)
HEAD_N = (1, 255, 257)
MAX_DEPTHS = (1.0, 80.0, 0.5)
MINMAX_B = (1, 3, 4, 5, 16, 17)
MINMAX_N = (1, 3, 4, 5, 255, 1027, 70001)
MINMAX_KINDS = ("mixed", "negative", "zeros", "subnormal", "huge", "const0", "const", "below", "above")
MINMAX_KIND_SHAPES = ((3, 1027), (4, 1028))  # later images misaligned (scalar path) | every image aligned (16-byte path without a tail)
TVPRE_N = (1, 255, 256, 257)
BFHALF_HW = ((2, 2), (2, 8), (4, 6), (6, 10), (64, 96))
BFPATCH_GRIDS = ((1, 1), (2, 2), (3, 3), (2, 4), (4, 4), (8, 8))  # (gw, gh): CP = 3, 12, 27, 24, 48, 192
BFPATCH_HW = ((5, 7), (8, 12))
SAM_RESIZES = {"up": (16, 16, 64, 64), "down": (64, 48, 40, 24), "identity": (24, 20, 24, 20), "dw1": (8, 8, 1, 5), "sw1": (1, 6, 7, 9),
               "wide": (20, 12, 30, 40), "tall": (12, 20, 40, 30)}  # (sw, sh, dw, dh)


def _patches_cases():
    out = []
    for ps, Kp in PATCH_SIZES:
        grids = PATCH_GRIDS + ((PATCH_BIG_GRIDS[ps],) if ps in PATCH_BIG_GRIDS else ())
        for ph, pw in grids:
            for B in (1, 3):
                for kind in ("ramp", "random"):
                    for norm in NORMS:
                        out.append(dict(id=f"patches-ps{ps}-kp{Kp}-{ph}x{pw}-b{B}-{kind}-{norm}", entry="patches", kind=kind, ps=ps, Kp=Kp, B=B, H=ph * ps, W=pw * ps, norm=norm))
    return out


def _pre32_cases():
    return [dict(id=f"pre32-b{B}-{H}x{W}-{norm}", entry="pre32", kind="ramp" if H * W < 256 else "random", B=B, H=H, W=W, norm=norm) for B, H, W in PRE32_SHAPES for norm in NORMS]


def _cls_cases():
    return [dict(id=f"cls-b{B}-t{T}-c{C}", entry="cls", kind="normal", B=B, T=T, C=C) for B in CLS_B for T in CLS_T for C in CLS_C]


def _head_out_cases():
    out = []
    for C in HEAD_OUT_WIDTHS:
        for n in HEAD_N:
            for md in MAX_DEPTHS:
                out.append(dict(id=f"headout-c{C}-n{n}-md{md:g}", entry="head_out", kind="mixed", C=C, n=n, max_depth=md, bias=0.3 if len(out) & 1 else -0.3))
        out.append(dict(id=f"headout-c{C}-n257-negative", entry="head_out", kind="negative", C=C, n=257, max_depth=80.0, bias=-0.3))
    out.append(dict(id=f"headout-c8-n{STRIDE_LOOP_N}-loop", entry="head_out", kind="mixed", C=8, n=STRIDE_LOOP_N, max_depth=80.0, bias=0.3))
    return out


def _minmax_cases():
    out = [dict(id=f"minmax-b{B}-n{n}-mixed", entry="minmax", kind="mixed", B=B, n=n, turn=i) for i, (B, n) in enumerate((B, n) for B in MINMAX_B for n in MINMAX_N)]
    for B, n in MINMAX_KIND_SHAPES:
        for i, kind in enumerate(MINMAX_KINDS):
            out.append(dict(id=f"minmax-b{B}-n{n}-{kind}-kinds", entry="minmax", kind=kind, B=B, n=n, turn=i))
    return out


def u8_values():
    """for every k the f32 nearest k / 255 with two neighbours on each side; negatives, values above 1, infinities, NaN, both zeros"""
    centre = (np.arange(256) / 255.0).astype(F32)
    lo1, hi1 = np.nextafter(centre, F32(-1)), np.nextafter(centre, F32(2))
    lo2, hi2 = np.nextafter(lo1, F32(-1)), np.nextafter(hi1, F32(2))
    special = np.array([-1.0, -1e-30, -0.0, 0.0, 1e-45, 0.5, 1.0000001, 2.0, 1e30, np.inf, -np.inf, np.nan], F32)
    return np.concatenate([np.stack([lo2, lo1, centre, hi1, hi2], axis=1).reshape(-1), special])


U8_CHUNK = 257


def _u8_cases():
    n_values = u8_values().size
    out = [dict(id=f"u8-n1-{name}", entry="u8", kind="special", n=1, value=v) for name, v in (("nan", np.nan), ("negzero", -0.0), ("one", 1.0))]
    out += [dict(id=f"u8-n{U8_CHUNK}-part{i}", entry="u8", kind="boundaries", n=U8_CHUNK, part=i) for i in range(-(-n_values // U8_CHUNK))]
    out.append(dict(id=f"u8-n{STRIDE_LOOP_N}-loop", entry="u8", kind="boundaries", n=STRIDE_LOOP_N, part=None))
    return out


def _tvpre_cases():
    return [dict(id=f"tvpre-n{n}-{kind}", entry="tvpre", kind=kind, n=n) for n in TVPRE_N for kind in ("ramp", "random")]


def _bfhalf_cases():
    return [dict(id=f"bfhalf-b{B}-{H}x{W}-{kind}", entry="bfhalf", kind=kind, B=B, H=H, W=W) for H, W in BFHALF_HW for B in (1, 2) for kind in ("random", "ramp")]


def _bfpatches_cases():
    return [dict(id=f"bfpatches-g{gw}x{gh}-{h}x{w}-b{B}", entry="bfpatches", kind="ramp" if gw * gh * h * w >= 256 else "random", gw=gw, gh=gh, h=h, w=w, B=B)
            for gw, gh in BFPATCH_GRIDS for h, w in BFPATCH_HW for B in (1, 2)]


def _sam_cases():
    return [dict(id=f"sam-{name}-{'f16' if f16 else 'f32'}-{'u8' if u8 else 'f32'}", entry="sam", kind="normal", resize=name, src_f16=f16, out_u8=u8)
            for name in SAM_RESIZES for f16 in (1, 0) for u8 in (0, 1)]


GROUPS = {"patches": _patches_cases(), "pre32": _pre32_cases(), "cls": _cls_cases(), "head_out": _head_out_cases(), "minmax": _minmax_cases(), "u8": _u8_cases(),
          "tvpre": _tvpre_cases(), "bfhalf": _bfhalf_cases(), "bfpatches": _bfpatches_cases(), "sam": _sam_cases()}
assert len({c["id"] for g in GROUPS.values() for c in g}) == sum(len(g) for g in GROUPS.values())
assert all(c["entry"] == name for name, g in GROUPS.items() for c in g)


def group(name):
    return GROUPS[name]


def all_cases():
    return [c for g in GROUPS.values() for c in g]


def case(cid):
    return next(c for c in all_cases() if c["id"] == cid)


# ---- materialize ------------------------------------------------------------------------------------------------------------------------------

def image(kind, B, n_pix, rng):
    """u8 [B, n_pix, 3]"""
    if kind == "random":
        return rng.integers(0, 256, (B, n_pix, 3), dtype=np.uint8)
    assert kind == "ramp"
    i, b, c = np.arange(n_pix)[None, :, None], np.arange(B)[:, None, None], np.arange(3)[None, None, :]
    return ((37 * i + 85 * c + 11 * b) % 256).astype(np.uint8)


def norm_of(name):
    """(mean, inv_std) f32 [3] as the caller hands them to the launcher"""
    if name == "identity":
        return np.zeros(3, F32), np.ones(3, F32)
    return R.IMAGENET_MEAN.copy(), R.IMAGENET_INV.copy()


def extreme_positions(n):
    """where an extreme is planted: the first element, the last element of the 16-byte body, the tail's last element, the middle"""
    return sorted({0, n - 1, n // 2} | ({4 * (n // 4) - 1} if n >= 4 else set()))


def planted(c, b):
    """(position of the minimum, of the maximum) of image b"""
    P = extreme_positions(c["n"])
    return P[(b + c["turn"]) % len(P)], P[(b + c["turn"] + 1) % len(P)]


def _minmax_data(c, rng):
    B, n, kind = c["B"], c["n"], c["kind"]
    d = np.empty((B, n), F32)
    below = np.nextafter(F32(1e-5), F32(0))
    for b in range(B):
        z = rng.standard_normal(n)
        pmin, pmax = planted(c, b)
        if kind in ("mixed", "negative", "huge"):
            v = 1.5 * z + 0.2 * b if kind != "negative" else -1.0 - np.abs(z) * (b + 1)
            v[pmax] = (v.max() if kind == "negative" else max(v.max(), 0.0)) + 0.25
            v[pmin] = min(v.min(), 0.0) - (1.0 + b)
            d[b] = v * (1e30 if kind == "huge" else 1.0)
        elif kind == "zeros":
            v = (np.abs(z) + 0.5).astype(F32)
            v[::7] = 0.0
            v[3::7] = -0.0
            d[b] = v
        elif kind == "subnormal":
            d[b] = (rng.integers(1, 1 << 22, n) * rng.choice([-1, 1], n)).astype(np.float64) * 2.0 ** -149
        elif kind in ("const0", "const"):
            d[b] = 0.0 if kind == "const0" else 3.25 + b
        else:
            top = below if kind == "below" else F32(1e-5)
            v = np.minimum((rng.uniform(0, 1, n) * float(top)).astype(F32), top)
            v[pmax], v[pmin] = top, 0.0
            d[b] = v
    return d


def _sam_plane(sh, sw, rng):
    """mask logits of both signs: standard normal, the first row positive and the last negative (a thresholded output holds both bytes)"""
    v = rng.standard_normal((sh, sw))
    v[0], v[-1] = np.abs(v[0]), -np.abs(v[-1])
    return v


def _sam_args(c, rng):
    sw, sh, dw, dh = SAM_RESIZES[c["resize"]]
    a = dict(src_f16=c["src_f16"], sw=sw, sh=sh, dw=dw, dh=dh, out_u8=c["out_u8"])
    if c["src_f16"]:  # column 2 of a [pixels][8] buffer; the other columns are not the call's to read
        buf = np.full((sh * sw, 8), np.nan, np.float16)
        buf[:, 2] = _sam_plane(sh, sw, rng).reshape(-1).astype(np.float16)
        a.update(src=buf, sstride=sw, step=8, offset=2)
    else:             # rows of sw + 3 elements; what lies between the rows is not the call's to read
        buf = np.full((sh, sw + 3), np.nan, F32)
        buf[:, :sw] = _sam_plane(sh, sw, rng).astype(F32)
        a.update(src=buf, sstride=sw + 3, step=1, offset=0)
    return a


def materialize(c) -> dict:
    rng = np.random.default_rng(zlib.crc32(c["id"].encode()))
    e = c["entry"]
    if e in ("patches", "pre32"):
        mean, inv = norm_of(c["norm"])
        a = dict(rgb=image(c["kind"], c["B"], c["H"] * c["W"], rng), B=c["B"], H=c["H"], W=c["W"], mean=mean, inv=inv)
        if e == "patches":
            a.update(ps=c["ps"], Kp=c["Kp"])
        return a
    if e == "cls":
        B, T, C = c["B"], c["T"], c["C"]
        return dict(B=B, T=T, C=C, x=rng.standard_normal((B * T, C)).astype(F32), cls=rng.standard_normal(C).astype(F32), pos=rng.standard_normal(T * C).astype(F32))
    if e == "head_out":
        n, C = c["n"], c["C"]
        if c["kind"] == "negative":  # x > 0, w < 0, bias < 0: every pre-activation is negative beyond its error
            x, w = np.abs(rng.standard_normal((n, C), dtype=F32)) + F32(0.1), -np.abs(rng.standard_normal(C)) - 0.05
        else:                        # x as a ReLU leaves it, weights of both signs: pre-activations of both signs
            x, w = np.maximum(rng.standard_normal((n, C), dtype=F32), 0), rng.standard_normal(C) * 0.3
        return dict(n=n, C=C, x=x.astype(np.float16), w=w.astype(F32), bias=c["bias"], max_depth=c["max_depth"])
    if e == "minmax":
        return dict(B=c["B"], n=c["n"], d=_minmax_data(c, rng))
    if e == "u8":
        if c["kind"] == "special":
            return dict(n=1, src=np.array([c["value"]], F32))
        values = u8_values()
        if c["part"] is None:
            return dict(n=c["n"], src=np.resize(values, c["n"]))
        return dict(n=c["n"], src=np.resize(np.roll(values, -c["part"] * U8_CHUNK), c["n"]))
    if e == "tvpre":
        return dict(n=c["n"], rgb=image(c["kind"], 1, c["n"], rng)[0])
    if e == "bfhalf":
        return dict(B=c["B"], H=c["H"], W=c["W"], rgb=image(c["kind"], c["B"], c["H"] * c["W"], rng))
    if e == "bfpatches":
        return dict(B=c["B"], h=c["h"], w=c["w"], gw=c["gw"], gh=c["gh"], rgb=image(c["kind"], c["B"], c["gh"] * c["h"] * c["gw"] * c["w"], rng))
    assert e == "sam"
    return _sam_args(c, rng)


def guard_of(c, a) -> int:
    return R.min_guard(c["entry"], a)


# ---- the refusals: (fields changed from an accepted base call, message fragment); nothing here is built to fault ---------------------------
# Pointer fields hold 1 (the scratch buffer), 2 (host memory: the launcher itself reads mean and inv_std) or 0 (NULL). Every base call, and
# every call of the tables should its refusal regress, stays inside the scratch buffer (65536 images: a grid the runtime refuses, or, for the
# cls rows, 65536 rows of one element).

_NULL = "null operand"
PATCHES_BASE = dict(rgb=1, out=1, mean=2, inv=2, B=1, H=8, W=8, ps=8, Kp=192)
_PATCHES_EMPTY = "vx_preprocess_patches: empty extent"
PATCHES_REFUSALS = ([(dict(**{k: 0}), "vx_preprocess_patches: " + _NULL) for k in ("rgb", "out", "mean", "inv")]
                    + [(f, _PATCHES_EMPTY) for f in (dict(ps=0), dict(ps=-8), dict(ps=-1), dict(B=0), dict(B=-1), dict(H=0), dict(W=0), dict(H=-8))]
                    + [(dict(B=65536), "65536 images do not fit the grid"), (dict(H=12), "8x12 not a multiple of patch size 8"), (dict(W=9), "9x8 not a multiple of patch size 8"),
                       (dict(Kp=100), "bad Kp=100"), (dict(Kp=184), "bad Kp=184"), (dict(Kp=0), "bad Kp=0")])
PRE32_BASE = dict(rgb=1, out=1, mean=2, inv=2, B=1, H=4, W=4)
PRE32_REFUSALS = ([(dict(**{k: 0}), "vx_preprocess_f32: " + _NULL) for k in ("rgb", "out", "mean", "inv")]
                  + [(f, "vx_preprocess_f32: empty extent") for f in (dict(B=0), dict(H=0), dict(W=0), dict(W=-1), dict(B=-2))])
CLS_BASE = dict(x=1, cls=1, pos=1, B=2, T=2, C=4)
CLS_REFUSALS = ([(dict(**{k: 0}), "vx_write_cls_rows: " + _NULL) for k in ("x", "cls", "pos")]
                + [(f, "vx_write_cls_rows: empty extent") for f in (dict(B=0), dict(B=-1), dict(T=0), dict(T=-1), dict(C=0), dict(C=-4))]
                + [(dict(B=65536, T=1, C=1), "65536 images do not fit the grid")])
HEAD_OUT_BASE = dict(x=1, w=1, depth=1, n=4, C=8)
HEAD_OUT_REFUSALS = ([(dict(**{k: 0}), "vx_head_out_f32: " + _NULL) for k in ("x", "w", "depth")]
                     + [(dict(n=0), "vx_head_out_f32: empty extent"), (dict(n=-5), "vx_head_out_f32: empty extent")]
                     + [(dict(C=C), f"vx_head_out_f32: unsupported C={C}") for C in (0, 4, 12, 24, 48, 128, -8)])
MINMAX_BASE = dict(depth=1, out=1, minmax=1, B=2, n=5)
MINMAX_REFUSALS = ([(dict(**{k: 0}), "vx_minmax_normalize: " + _NULL) for k in ("depth", "out", "minmax")]
                   + [(f, "vx_minmax_normalize: empty extent") for f in (dict(B=0), dict(B=-1), dict(n=0), dict(n=-1))]
                   + [(dict(B=65536, n=1), "65536 images do not fit the grid")])
U8_BASE = dict(src=1, dst=1, n=16)
U8_REFUSALS = [(dict(src=0), "vx_f32_to_u8: " + _NULL), (dict(dst=0), "vx_f32_to_u8: " + _NULL), (dict(n=0), "vx_f32_to_u8: empty extent"), (dict(n=-1), "vx_f32_to_u8: empty extent")]
TVPRE_BASE = dict(rgb=1, out=1, n=4)
TVPRE_REFUSALS = [(f, "vx_tv_preprocess: bad operands") for f in (dict(rgb=0), dict(out=0), dict(n=0), dict(n=-1))]
BFHALF_BASE = dict(rgb=1, out=1, B=1, H=4, W=6)
BFHALF_REFUSALS = ([(f, "vx_bf_preprocess_half: bad operands") for f in (dict(rgb=0), dict(out=0), dict(B=0))]
                   + [(dict(H=3), "extent 6x3 must be even"), (dict(W=5), "extent 5x4 must be even"), (dict(H=0), "extent 6x0 must be even"), (dict(W=0), "extent 0x4 must be even")])
BFPATCHES_BASE = dict(rgb=1, out=1, B=1, IH=8, IW=12, h=4, w=6)
BFPATCHES_REFUSALS = ([(f, "vx_bf_patches: grid") for f in (dict(rgb=0), dict(out=0), dict(B=0), dict(h=0), dict(w=0), dict(IH=0), dict(IW=0), dict(h=-4))]
                      + [(dict(h=3), "grid 6x3 must divide the image 12x8"), (dict(w=5), "grid 5x4 must divide the image 12x8")])
SAM_BASE = dict(src=1, src_f16=0, sw=4, sh=4, sstride=4, step=1, dst=1, dw=8, dh=8, out_u8=0)
SAM_REFUSALS = [(f, "vx_sam_interpolate: bad operands") for f in (dict(src=0), dict(dst=0), dict(sw=0), dict(sh=0), dict(dw=0), dict(dh=0), dict(step=0), dict(step=-1),
                                                                  dict(sstride=3), dict(sw=-4, sstride=-4), dict(src_f16=1, dw=0), dict(out_u8=1, dh=-1))]
REFUSAL_TABLES = {"patches": PATCHES_REFUSALS, "pre32": PRE32_REFUSALS, "cls": CLS_REFUSALS, "head_out": HEAD_OUT_REFUSALS, "minmax": MINMAX_REFUSALS, "u8": U8_REFUSALS,
                  "tvpre": TVPRE_REFUSALS, "bfhalf": BFHALF_REFUSALS, "bfpatches": BFPATCHES_REFUSALS, "sam": SAM_REFUSALS}
REFUSAL_BASES = {"patches": PATCHES_BASE, "pre32": PRE32_BASE, "cls": CLS_BASE, "head_out": HEAD_OUT_BASE, "minmax": MINMAX_BASE, "u8": U8_BASE, "tvpre": TVPRE_BASE,
                 "bfhalf": BFHALF_BASE, "bfpatches": BFPATCHES_BASE, "sam": SAM_BASE}
N_REFUSALS = sum(len(t) for t in REFUSAL_TABLES.values())
REFUSAL_SCRATCH_BYTES = 1 << 20
ENTRY_POINT = {"patches": "vx_preprocess_patches", "pre32": "vx_preprocess_f32", "cls": "vx_write_cls_rows", "head_out": "vx_head_out_f32", "minmax": "vx_minmax_normalize",
               "u8": "vx_f32_to_u8", "tvpre": "vx_tv_preprocess", "bfhalf": "vx_bf_preprocess_half", "bfpatches": "vx_bf_patches", "sam": "vx_sam_interpolate"}


def float3(v):
    """a host array of three floats as the launchers of kernels_misc.hip read mean and inv_std"""
    return (ctypes.c_float * 3)(*[float(t) for t in v])


def call(lib, entry, f, p):
    """one call of launcher `entry` with the fields f; p(field) turns a pointer field into an address or NULL"""
    if entry == "patches":
        return lib.vx_preprocess_patches(p(f["rgb"]), p(f["out"]), f["B"], f["H"], f["W"], f["ps"], f["Kp"], p(f["mean"]), p(f["inv"]), None)
    if entry == "pre32":
        return lib.vx_preprocess_f32(p(f["rgb"]), p(f["out"]), f["B"], f["H"], f["W"], p(f["mean"]), p(f["inv"]), None)
    if entry == "cls":
        return lib.vx_write_cls_rows(p(f["x"]), p(f["cls"]), p(f["pos"]), f["B"], f["T"], f["C"], None)
    if entry == "head_out":
        return lib.vx_head_out_f32(p(f["x"]), p(f["w"]), f.get("bias", 0.0), f.get("max_depth", 1.0), p(f["depth"]), f["n"], f["C"], None)
    if entry == "minmax":
        return lib.vx_minmax_normalize(p(f["depth"]), p(f["out"]), p(f["minmax"]), f["B"], f["n"], None)
    if entry == "u8":
        return lib.vx_f32_to_u8(p(f["src"]), p(f["dst"]), f["n"], None)
    if entry == "tvpre":
        return lib.vx_tv_preprocess(p(f["rgb"]), p(f["out"]), f["n"], None)
    if entry == "bfhalf":
        return lib.vx_bf_preprocess_half(p(f["rgb"]), p(f["out"]), f["B"], f["H"], f["W"], None)
    if entry == "bfpatches":
        return lib.vx_bf_patches(p(f["rgb"]), p(f["out"]), f["B"], f["IH"], f["IW"], f["h"], f["w"], None)
    assert entry == "sam"
    return lib.vx_sam_interpolate(p(f["src"]), f["src_f16"], f["sw"], f["sh"], f["sstride"], f["step"], p(f["dst"]), f["dw"], f["dh"], f["out_u8"], None)


def run_refusals(lib, ptr, host_ptr, seen=None):
    """every table entry against the library: returns 0 with its message (before any launch: `ptr` is never dereferenced) -> the number run;
    `seen` collects (entry, message)"""
    n = 0
    for entry, table in REFUSAL_TABLES.items():
        for fields, message in table:
            f = dict(REFUSAL_BASES[entry], **fields)
            r = call(lib, entry, f, lambda flag: (None, ptr, host_ptr)[flag])
            assert r == 0 and message.encode() in lib.vx_last_error(), (entry, fields, message, lib.vx_last_error())
            if seen is not None:
                seen.append((entry, lib.vx_last_error().decode()))
            n += 1
    return n


def run_base_calls(lib, ptr, host_ptr):
    """the base call of every table is accepted (on a scratch of its own: these calls launch) -> the number run"""
    for entry, base in REFUSAL_BASES.items():
        assert call(lib, entry, base, lambda flag: (None, ptr, host_ptr)[flag]) == 1, (entry, lib.vx_last_error())
    return len(REFUSAL_BASES)

"""The case tables of the sampling and halo matrix-core kernels' argument space -- vx_deform_conv_f16 (`deform`), vx_bf_deform_cols_f16 (`cols`),
vx_mbconv_dw_pw_f16 (`mbconv`), vx_conv3x3_f16 (`halo`) -- built the same way by the CPU tests that check their completeness
(tests/test_sampled_ref_cpu.py) and by the GPU tests that run them (tests/test_gpu_sampled_matrix.py). A case is a small dict of data only;
`materialize` turns it into the `args` dict of tests/sampled_ref.py with whole buffers, operands already rounded to the stored type, seeded by
the case id. The launchers' host-side decisions are restated here from csrc/kernels_deform.hip and csrc/kernels_mbconv.hip."""
from __future__ import annotations

import zlib

import numpy as np

import gemm_ref as G
import sampled_ref as R

# ---- the launchers, restated ----------------------------------------------------------------------------------------------------------------


def deform_ck(cin) -> int:
    """vx_deform_conv_f16's instantiation: channels of one tap per k step"""
    return 64 if cin % 64 == 0 else 48 if cin % 48 == 0 else 32 if cin % 32 == 0 else 16


def deform_extent(c):
    return c["H"] + 2 * c["pad"] - c["k"] + 1, c["W"] + 2 * c["pad"] - c["k"] + 1


def deform_m(c) -> int:
    OH, OW = deform_extent(c)
    return c["B"] * OH * OW


def mbconv_blocks(c) -> int:
    return c["B"] * c["H"] * (c["W"] // R.MB_PX)


# ---- deform cases -------------------------------------------------------------------------------------------------------------------------------

DEFORM_BASE = dict(entry="deform", kind="random", B=2, H=5, W=7, Cin=16, Cout=32, k=3, pad=1, mask_mode=1, mask_scale=2.0, epi="", ld_offset="pad8", ldo=8, out_off=0)
CINS = (16, 80, 32, 160, 48, 96, 64, 128)  # CK 16, 16, 32, 32, 48, 48, 64, 64 with 1, 5, 1, 5, 1, 2, 1, 2 steps per tap
K_PAD = [(1, 0), (2, 0), (2, 1), (3, 0), (3, 2), (4, 1), (5, 2), (6, 3), (7, 3), (7, 0)]  # on a 7 x 9 map: OH below, equal to and above H
COUTS = (8, 32, 40, 128, 136, 256)
M_CLASSES = {9: dict(B=1, H=3, W=3), 33: dict(B=1, H=3, W=11), 64: dict(B=1, H=8, W=8), 65: dict(B=1, H=5, W=13), 70: dict(B=2, H=5, W=7), 192: dict(B=3, H=8, W=8)}
EPILOGUES = ("", "s", "b", "r", "sbr")  # scale, bias, relu
PLANTS = ("py=-1", "py=H", "py=H-1/2", "px=-1/2", "px=W-1/2", "integer", "far")
IMPULSE_HOT = (2, 3)  # the one-hot input pixel (y, x) of the impulse cases, in the last image
IMPULSE_OUT = (2, 2)  # the one output pixel whose tap samples next to it
IMPULSE_FRAC = (0.25, 0.75)


def _deform(cid, **fields):
    c = dict(DEFORM_BASE, id=cid, **fields)
    assert deform_m(c) < 400
    return c


def _deform_cases():
    out = []
    for kind, tag in (("random", ""), ("positive", "-pos")):
        for cin in CINS:
            out.append(_deform(f"deform-cin{cin}{tag}", kind=kind, Cin=cin))
        for k, pad in K_PAD:
            out.append(_deform(f"deform-k{k}p{pad}{tag}", kind=kind, k=k, pad=pad, H=7, W=9))
        out.append(_deform(f"deform-k7p3-4x6{tag}", kind=kind, k=7, pad=3, H=4, W=6))  # the kernel is larger than the map
        for cout in COUTS:
            out.append(_deform(f"deform-cout{cout}{tag}", kind=kind, Cin=32, k=1, pad=0, Cout=cout))
        for m, shape in M_CLASSES.items():
            out.append(_deform(f"deform-m{m}{tag}", kind=kind, **shape))
    out.append(_deform("deform-mask0", mask_mode=0))
    out.append(_deform("deform-mask1-separate", mask_mode=1))
    for ms in (2.0, 1.0, 0.5):
        out.append(_deform(f"deform-mask2-scale{ms:g}", mask_mode=2, mask_scale=ms))
    out.append(_deform("deform-mask2-pos", kind="positive", mask_mode=2, Cin=48))
    for epi in EPILOGUES:
        out.append(_deform(f"deform-epi-{epi or 'none'}", epi=epi))
        out.append(_deform(f"deform-epi-{epi or 'none'}-pos", kind="positive", epi=epi, Cout=40))
    for ld in ("exact", "odd", "pad8"):
        out.append(_deform(f"deform-ldoffset-{ld}", ld_offset=ld))
    out.append(_deform("deform-ldoffset-odd-mask2", ld_offset="odd", mask_mode=2))
    out.append(_deform("deform-ldo-cout", ldo=0))
    out.append(_deform("deform-ldo-cout+4-shifted", ldo=4, out_off=4))  # `out` 8-byte but not 16-byte aligned, rows of Cout + 4
    out.append(_deform("deform-ldo-cout+8", ldo=8))
    out.append(_deform("deform-zero-offset", kind="zero-offset", mask_mode=0))
    out.append(_deform("deform-zero-offset-k4p1-cin48", kind="zero-offset", mask_mode=0, k=4, pad=1, Cin=48, H=7, W=9))
    for tap in range(9):
        for corner in range(4):
            out.append(_deform(f"deform-impulse-tap{tap}-corner{corner}", kind="impulse", tap=tap, corner=corner))
    out.append(_deform("deform-far", kind="far"))
    out.append(_deform("deform-far-k7p3-cin48", kind="far", k=7, pad=3, Cin=48, mask_mode=0))
    return out


# ---- cols cases ---------------------------------------------------------------------------------------------------------------------------------

def _cols_cases():
    out = []
    for C in (8, 24, 64):
        for k in (1, 3, 7):
            for ld in ("exact", "pad8"):
                for kind, tag in (("random", ""), ("positive", "-pos")):
                    out.append(dict(id=f"cols-c{C}-k{k}-{ld}{tag}", entry="cols", kind=kind, B=2, H=5, W=7, C=C, k=k, ldom=ld))
    for tap in range(9):
        for corner in range(4):
            out.append(dict(id=f"cols-impulse-tap{tap}-corner{corner}", entry="cols", kind="impulse", B=2, H=5, W=7, C=8, k=3, ldom="exact", tap=tap, corner=corner))
    return out


# ---- mbconv cases -------------------------------------------------------------------------------------------------------------------------------

MB_SHAPES = [(1, 1, 64), (1, 2, 64), (2, 3, 64), (1, 9, 64), (3, 5, 64), (1, 8, 128), (2, 5, 192)]  # 1, 2, 6, 9, 15, 16 and 30 blocks
MB_IMPULSE = dict(B=2, H=3, W=128)   # two segments per row: the x = 63 | 64 seam lies inside the map
MB_IMPULSE_AT = ((1, 64), (1, 8))    # (y, x) of the two one-hot pixels: next to the segment seam, next to a strip seam
W3_PROBE_B2 = 12.0                   # gelu(12 + d) = 12 + d exactly, in float64 and in f32: both GELUs are the identity, and 12 + d is an f16 value


def w3_probe_column(n):
    return (37 * n + 5) % 256


def _mbconv_cases():
    out = []
    for B, H, W in MB_SHAPES:
        for kind, tag in (("random", ""), ("positive", "-pos")):
            out.append(dict(id=f"mbconv-{B}x{H}x{W}{tag}", entry="mbconv", kind=kind, B=B, H=H, W=W))
    for tap in range(9):
        out.append(dict(MB_IMPULSE, id=f"mbconv-impulse-tap{tap}", entry="mbconv", kind="impulse", tap=tap))
    out.append(dict(id="mbconv-w3-probe", entry="mbconv", kind="w3-probe", B=2, H=3, W=64))
    out.append(dict(id="mbconv-zero-bias", entry="mbconv", kind="random", B=2, H=3, W=64, zero_bias=True))
    return out


# ---- halo cases ---------------------------------------------------------------------------------------------------------------------------------

HALO_MAPS = [(1, 1), (8, 32), (9, 33), (3, 70)]
HALO_EPILOGUES = {  # name -> (epilogue, relu, res1, res2)
    "f16": (G.F16, 0, 0, 0), "relu": (G.RELU, 0, 0, 0), "add": (G.ADD, 0, 0, 0), "add-res1": (G.ADD, 0, 1, 0), "add-res12": (G.ADD, 0, 1, 1),
    "add-relu-res1": (G.ADD, 1, 1, 0), "head": (G.HEAD_OUT, 0, 0, 0)}


def _halo(cid, cin, cout, H, W, epi, a_relu=0, kind="random", bias=True, k_extra=0):
    return dict(id=cid, entry="halo", kind=kind, B=2, H=H, W=W, cin=cin, cout=cout, epi=epi, a_relu=a_relu, bias=bias, k_extra=k_extra)


def _halo_cases():
    out, i = [], 0
    for cin in (32, 64):
        for cout in (32, 64):
            for H, W in HALO_MAPS:
                for epi in HALO_EPILOGUES:
                    if epi == "head" and cout != 32:
                        continue
                    i += 1
                    for a_relu in ((0, 1) if (H, W) == (9, 33) else (i & 1,)):  # both values on the ragged map, alternating elsewhere
                        out.append(_halo(f"halo-{cin}-{cout}-{H}x{W}-{epi}" + ("-arelu" if a_relu else ""), cin, cout, H, W, epi, a_relu))
                    if (H, W) == (9, 33):
                        out.append(_halo(f"halo-{cin}-{cout}-{H}x{W}-{epi}-pos", cin, cout, H, W, epi, kind="positive"))
            out.append(_halo(f"halo-{cin}-{cout}-nobias", cin, cout, 9, 33, "f16", bias=False))
            out.append(_halo(f"halo-{cin}-{cout}-nobias-add", cin, cout, 3, 70, "add-res12", a_relu=1, bias=False))
    out.append(_halo("halo-32-64-k-extra", 32, 64, 9, 33, "relu", k_extra=64))  # K = 9 cin rounded up to 64 and 64 more: pad columns the kernel must not read
    out.append(_halo("halo-64-32-k-extra-head", 64, 32, 9, 33, "head", k_extra=64))
    return out


GROUPS = {"deform": _deform_cases(), "cols": _cols_cases(), "mbconv": _mbconv_cases(), "halo": _halo_cases()}
assert len({c["id"] for g in GROUPS.values() for c in g}) == sum(len(g) for g in GROUPS.values())


def group(name):
    return GROUPS[name]


def all_cases():
    return [c for g in GROUPS.values() for c in g]


def case(cid):
    return next(c for c in all_cases() if c["id"] == cid)


# ---- materialize ------------------------------------------------------------------------------------------------------------------------------

def _f16(a):
    return np.asarray(a).astype(np.float16)


def plant(off, H, W, k, pad, rng):
    """Plants the positions of PLANTS into the offsets [B, OH, OW, 2 taps] (in place) for the first and the last tap, each on a (pixel, tap) of
    its own -> [(what, tap, b, oy, ox)]. Every planted offset is an integer or a half of small magnitude: exact in f16,
    and the f32 position sum is exact."""
    B, OH, OW, _ = off.shape
    taps = k * k
    pixels = rng.permutation(B * OH * OW)
    planted = []
    for i, end in enumerate(dict.fromkeys((0, taps - 1))):
        for j, what in enumerate(PLANTS):
            slot = i * len(PLANTS) + j
            tap = end + (j // pixels.size) * (1 if end == 0 else -1)  # a map with fewer pixels than plants: the next tap of the same pixel
            ky, kx = divmod(tap, k)
            b, rm = divmod(int(pixels[slot % pixels.size]), OH * OW)
            oy, ox = divmod(rm, OW)
            iy, ix = oy - pad + ky, ox - pad + kx
            if what == "py=-1":
                off[b, oy, ox, 2 * tap] = -1 - iy
            elif what == "py=H":
                off[b, oy, ox, 2 * tap] = H - iy
            elif what == "py=H-1/2":
                off[b, oy, ox, 2 * tap] = H - 0.5 - iy
            elif what == "px=-1/2":
                off[b, oy, ox, 2 * tap + 1] = -0.5 - ix
            elif what == "px=W-1/2":
                off[b, oy, ox, 2 * tap + 1] = W - 0.5 - ix
            elif what == "integer":
                off[b, oy, ox, 2 * tap:2 * tap + 2] = [(oy + 1) % H - iy, (ox + 2) % W - ix]
            else:
                off[b, oy, ox, 2 * tap:2 * tap + 2] = [-30, -4 - W - ix]
            if what in ("py=H-1/2", "px=-1/2", "px=W-1/2"):  # the other coordinate inside the map, so that the half-outside cell counts
                other = 2 * tap + (1 if what.startswith("py") else 0)
                off[b, oy, ox, other] = ((ox + 1) % W - ix) if what.startswith("py") else ((oy + 1) % H - iy)
            planted.append((what, tap, b, oy, ox))
    return planted


def _impulse(c, B, H, W, OH, OW, taps, C):
    """x one-hot at IMPULSE_HOT of the last image; every offset far outside but tap `tap` of output pixel IMPULSE_OUT, whose sample lies
    IMPULSE_FRAC behind the cell corner that makes the hot pixel its corner `corner` -> (x, offsets, the hot channel, the corner's weight)"""
    tap, corner = c["tap"], c["corner"]
    ch = (3 * tap + corner) % C
    x = np.zeros((B, H, W, C))
    x[B - 1, IMPULSE_HOT[0], IMPULSE_HOT[1], ch] = 1.5
    off = np.full((B, OH, OW, 2 * taps), -40.0)
    ky, kx = divmod(tap, 3)
    cy, cx = divmod(corner, 2)
    oy, ox = IMPULSE_OUT
    off[B - 1, oy, ox, 2 * tap] = IMPULSE_HOT[0] - cy + IMPULSE_FRAC[0] - (oy - 1 + ky)
    off[B - 1, oy, ox, 2 * tap + 1] = IMPULSE_HOT[1] - cx + IMPULSE_FRAC[1] - (ox - 1 + kx)
    ly, lx = IMPULSE_FRAC
    weight = ((1 - ly) * (1 - lx), (1 - ly) * lx, ly * (1 - lx), ly * lx)[corner]
    return x, off, ch, weight


def _sampler_data(c, rng, B, H, W, OH, OW, k, pad, C):
    """x, offsets, logits, planted for the data kinds the two samplers share"""
    taps, kind = k * k, c["kind"]
    x = rng.standard_normal((B, H, W, C))
    off = rng.standard_normal((B, OH, OW, 2 * taps)) * 1.2
    logits = rng.standard_normal((B, OH, OW, taps))
    planted = []
    if kind == "positive":
        x = np.abs(x)
    if kind == "zero-offset":
        off = np.zeros_like(off)
    elif kind == "far":
        off = rng.uniform(100, 2000, off.shape) * rng.choice([-1.0, 1.0], off.shape)
    elif kind != "impulse":
        off = _f16(off).astype(np.float64)
        planted = plant(off, H, W, k, pad, rng)
    return x, off, logits, planted


def _materialize_deform(c, rng):
    B, H, W, Cin, Cout, k, pad, kind, mode = (c[key] for key in ("B", "H", "W", "Cin", "Cout", "k", "pad", "kind", "mask_mode"))
    taps = k * k
    OH, OW = deform_extent(c)
    M = B * OH * OW
    x, off, logits, planted = _sampler_data(c, rng, B, H, W, OH, OW, k, pad, Cin)
    w = rng.standard_normal((Cout, taps, Cin)) / np.sqrt(taps * Cin)
    scale, bias = 1 + 0.3 * rng.standard_normal(Cout), 0.1 * rng.standard_normal(Cout)
    if "s" in c["epi"]:
        scale[1::5] *= -1  # a negative batch-norm weight as well
    mask = logits if mode == 2 else np.float64(c["mask_scale"]) * R.D.sigmoid(logits)  # mode 1: the factor itself, stored in f16
    info = {}
    if kind == "positive":
        w, bias = np.abs(w), np.abs(bias)
        scale = np.abs(scale)
    elif kind == "impulse":
        x, off, ch, weight = _impulse(c, B, H, W, OH, OW, taps, Cin)
        n = (5 * c["tap"] + 7 * c["corner"] + 1) % Cout
        w = np.zeros_like(w)
        w[n, c["tap"], ch] = 0.75
        mask = np.broadcast_to(0.5 + np.arange(taps) / 16.0, (B, OH, OW, taps)).copy()  # a factor of its own per tap
        info = dict(hot=(n, 1.5 * 0.75 * weight * (mask[0, 0, 0, c["tap"]] if mode else 1.0)))
    ld_offset = {"exact": 2 * taps, "odd": 2 * taps + 1, "pad8": -(-2 * taps // 8) * 8}[c["ld_offset"]]
    side_by_side = mode == 2  # offsets and logits in one buffer, as the offsets product leaves them
    if side_by_side:
        ld_offset = {"exact": 3 * taps, "odd": 3 * taps + (1 if taps % 2 == 0 else 2), "pad8": -(-3 * taps // 8) * 8}[c["ld_offset"]]
    om = np.full((M, ld_offset), np.nan, np.float16)  # what lies between the rows is not the call's to read
    om[:, :2 * taps] = _f16(off).reshape(M, -1)
    a = dict(B=B, H=H, W=W, Cin=Cin, Cout=Cout, k=k, pad=pad, mask_mode=mode, mask_scale=float(c["mask_scale"]), relu=int("r" in c["epi"]), ld_offset=ld_offset,
             ldo=Cout + c["ldo"], out_off=c["out_off"], mask=None, ld_mask=0, mask_col=0, planted=planted, **info)
    if side_by_side:
        om[:, 2 * taps:3 * taps] = _f16(mask).reshape(M, -1)
        a.update(mask_col=2 * taps, ld_mask=ld_offset)
    elif mode == 1:
        a.update(mask=_f16(mask).reshape(M, taps), ld_mask=taps)
    wp = np.zeros((-(-Cout // 32) * 32, taps * Cin), np.float16)  # the header: pad rows zero
    wp[:Cout] = _f16(w).reshape(Cout, -1)
    a.update(x=_f16(x), w=wp, offset=om, scale=scale.astype(np.float32) if "s" in c["epi"] else None, bias=bias.astype(np.float32) if "b" in c["epi"] else None)
    return a


def _materialize_cols(c, rng):
    B, H, W, C, k, kind = (c[key] for key in ("B", "H", "W", "C", "k", "kind"))
    taps, M = k * k, B * H * W
    x, off, logits, planted = _sampler_data(c, rng, B, H, W, H, W, k, k // 2, C)
    info = {}
    if kind == "impulse":
        x, off, ch, weight = _impulse(c, B, H, W, H, W, taps, C)
        logits = np.broadcast_to((np.arange(taps) - 4) / 4.0, (B, H, W, taps)).copy()
        info = dict(hot=(c["tap"] * C + ch, 1.5 * weight))  # times 2 sigmoid(logit of the tap)
    ldom = 3 * taps if c["ldom"] == "exact" else -(-3 * taps // 8) * 8
    om = np.full((M, ldom), np.nan, np.float16)
    om[:, :2 * taps], om[:, 2 * taps:3 * taps] = _f16(off).reshape(M, -1), _f16(logits).reshape(M, -1)
    return dict(B=B, H=H, W=W, C=C, k=k, ldom=ldom, x=_f16(x), om=om, planted=planted, **info)


def _materialize_mbconv(c, rng):
    B, H, W, kind = c["B"], c["H"], c["W"], c["kind"]
    h = rng.standard_normal((B, H, W, R.MB_C))
    w2 = rng.standard_normal((9, R.MB_C)) / 3
    b2, b3 = rng.standard_normal(R.MB_C) * 0.2, rng.standard_normal(R.MB_CO) * 0.2
    w3 = rng.standard_normal((R.MB_CO, R.MB_C)) / 16
    x = rng.standard_normal((B, H, W, R.MB_CO))
    if kind == "positive":
        h, w2, b2, w3, b3, x = (np.abs(v) for v in (h, w2, b2, w3, b3, x))
    elif kind == "impulse":  # two one-hot pixels, one depthwise tap, w3 = one row per hot channel: out(y, x) = in(y + ky - 1, x + kx - 1)
        tap = c["tap"]
        h, w2, w3 = np.zeros_like(h), np.zeros_like(w2), np.zeros_like(w3)
        b2, b3, x = np.zeros_like(b2), np.zeros_like(b3), np.zeros_like(x)
        for i, (y, xx) in enumerate(MB_IMPULSE_AT):
            ch = (29 * tap + 100 * i + 3) % R.MB_C
            h[B - 1, y, xx, ch] = 1.5
            w2[tap, ch] = 2.0
            w3[(7 * tap + 30 * i + 1) % R.MB_CO, ch] = 1.0
    elif kind == "w3-probe":  # output channel n reads depthwise channel (37 n + 5) % 256 alone, the inner GELU near the identity: it names its channel
        w3 = np.zeros_like(w3)
        w3[np.arange(R.MB_CO), w3_probe_column(np.arange(R.MB_CO))] = 1.0
        w2 = np.zeros_like(w2)
        w2[4] = 1.0
        h = np.broadcast_to(np.arange(R.MB_C) / 64.0, h.shape) + rng.integers(0, 2, h.shape[:3] + (1,)) / 128.0  # channel c holds c / 64 (+ a pixel's bit)
        b2, b3, x = np.full(R.MB_C, W3_PROBE_B2), np.zeros(R.MB_CO), np.zeros_like(x)
    if c.get("zero_bias"):
        b2, b3 = np.zeros_like(b2), np.zeros_like(b3)
    rows = _f16(w3)
    return dict(B=B, H=H, W=W, h=_f16(h), w2=_f16(w2), b2=b2.astype(np.float32), w3_rows=rows, w3=R.pack_w3(rows), b3=b3.astype(np.float32), x=_f16(x))


def _materialize_halo(c, rng):
    B, H, W, cin, cout, kind = (c[key] for key in ("B", "H", "W", "cin", "cout", "kind"))
    epi, relu, res1, res2 = HALO_EPILOGUES[c["epi"]]
    k_real = 9 * cin
    K = -(-k_real // 64) * 64 + c["k_extra"]
    M = B * H * W
    pos = np.abs if kind == "positive" else (lambda v: v)
    a = dict(conv_kh=3, conv_kw=3, conv_stride=1, conv_pad=1, conv_H=H, conv_W=W, conv_Cin=cin, conv_OH=H, conv_OW=W, M=M, N=cout, K=K, epi=epi, a_relu=c["a_relu"], A_off=0)
    a["A"] = _f16(pos(rng.standard_normal((B, H, W, cin))))
    Wm = np.full((cout, K), 512.0)  # the K padding holds values the kernel must not read
    Wm[:, :k_real] = pos(rng.standard_normal((cout, k_real))) / np.sqrt(k_real)
    a["W"] = _f16(Wm)
    a["bias"] = pos(rng.standard_normal(cout) * 0.1).astype(np.float32) if c["bias"] else None
    if epi == G.HEAD_OUT:
        a.update(ldo=1, lambda_=pos(rng.standard_normal(cout) * 0.3).astype(np.float32), head_bias=0.05, head_scale=2.0)
    else:
        a.update(ldo=cout + 8, relu=relu)
        if res1:
            a["res1"] = _f16(pos(rng.standard_normal((M, cout + 8))))
        if res2:
            a["res2"] = _f16(pos(rng.standard_normal((M, cout + 8))))
    return a


def materialize(c) -> dict:
    rng = np.random.default_rng(zlib.crc32(c["id"].encode()))
    return {"deform": _materialize_deform, "cols": _materialize_cols, "mbconv": _materialize_mbconv, "halo": _materialize_halo}[c["entry"]](c, rng)


def guard_of(c, a) -> int:
    return R.min_guard(c["entry"], a)


# ---- the refusals: (fields changed from an accepted base call, message fragment); nothing here is built to fault ---------------------------

DEFORM_REFUSAL_BASE = dict(x=1, w=1, offset=1, out=1, mask=1, scale=0, bias=0, B=1, H=5, W=7, Cin=16, Cout=32, k=3, pad=1, ld_offset=18, ld_mask=9, mask_mode=1, ldo=32,
                           out_shift=0, x_shift=0, scale_shift=0)
DEFORM_REFUSALS = ([(dict(**{k: 0}), "null operand") for k in ("x", "w", "offset", "out")]
                   + [(dict(Cin=24), "Cin = 24 must be a multiple of 16"), (dict(Cin=0), "must be a multiple of 16"), (dict(B=0), "must be a multiple of 16"), (dict(H=0), "must be a multiple of 16"),
                      (dict(Cout=12), "Cout = 12 (a multiple of 8, at most 256"), (dict(Cout=264), "Cout = 264"), (dict(Cout=0), "Cout = 0"),
                      (dict(k=0), "kernel 0, pad 1 (kernels 1..7)"), (dict(k=8, pad=4), "kernel 8, pad 4"), (dict(pad=-1), "kernel 3, pad -1"),
                      (dict(k=7, pad=0, H=5, W=7, ld_offset=98, ld_mask=49), "output extent 1x-1"), (dict(B=40000, H=300, W=300), "output extent"),
                      (dict(B=1 << 10, H=1 << 10, W=1 << 10, Cin=1 << 10), "input too large"),
                      (dict(ld_offset=17), "offset rows of 17 elements hold fewer than 2 x 9 taps"),
                      (dict(mask_mode=3), "mask mode 3"), (dict(mask_mode=-1), "mask mode -1"), (dict(mask=0), "mask mode 1"), (dict(ld_mask=8), "mask rows of 8 elements for 9 taps"),
                      (dict(mask_mode=2, mask=0), "mask mode 2"),
                      (dict(ldo=24), "output rows of 24 elements"), (dict(ldo=34), "output rows of 34 elements"), (dict(out_shift=4), "output rows of 32 elements"),
                      (dict(x_shift=8), "must be 16-byte aligned"), (dict(scale=1, scale_shift=4), "must be 16-byte aligned")])
MBCONV_REFUSAL_BASE = dict(h=1, w2=1, b2=1, w3=1, b3=1, x=1, y=1, B=1, H=2, W=64, C=256, Cout=64)
MBCONV_REFUSALS = ([(dict(**{k: 0}), "bad operands") for k in ("h", "w2", "b2", "w3", "b3", "x", "y")] + [(dict(B=0), "bad operands"), (dict(H=0), "bad operands")]
                   + [(dict(C=128), "C = 128, Cout = 64, W = 64"), (dict(Cout=32), "C = 256, Cout = 32, W = 64"), (dict(W=96), "W = 96"), (dict(W=32), "W = 32"), (dict(W=0), "W = 0")])
HALO_REFUSAL_BASE = dict(A=1, W=1, out=1, conv_kh=3, conv_kw=3, conv_stride=1, conv_pad=1, conv_H=8, conv_W=32, conv_Cin=32, conv_OH=8, conv_OW=32, M=256, N=32, K=320, epi=G.F16, ldo=32)
_SHAPE = "unsupported shape (3x3 s1 p1"
HALO_REFUSALS = ([(f, _SHAPE) for f in (dict(conv_kh=1), dict(conv_kw=5), dict(conv_stride=2), dict(conv_pad=0), dict(conv_Cin=16), dict(conv_Cin=128, K=1152), dict(N=128), dict(N=48),
                                        dict(n_valid=24), dict(conv_OH=6), dict(conv_OW=30), dict(epi=G.GELU), dict(epi=G.SILU), dict(epi=G.HEAD_OUT, N=64, lambda_=1))]
                 + [(dict(conv_pix=64), "conv_pix"), (dict(conv_pix=40), "conv_pix"), (dict(epi=G.ADD, res1=1, post_gelu=1), "post_gelu"), (dict(epi=G.ADD, res1=1, win_ws=8, win_res=32), "window-order"),
                    (dict(win_res_h=8), "window-order"), (dict(k_splits=2), "k_splits"), (dict(epi=G.ADD, res1=1, ld_res1=40), "ld_res1"), (dict(a_group=4), "a_group"), (dict(epi=G.ADD, res2=1), "res2 without res1"),
                    (dict(K=256), "bad operands"), (dict(A=0), "bad operands"), (dict(W=0), "bad operands"), (dict(out=0), "bad operands"), (dict(M=250), "not a whole number of images"),
                    (dict(M=0), "not a whole number of images"), (dict(ldo=36), "ldo=36"), (dict(ldo=24), "ldo=24"), (dict(epi=G.HEAD_OUT, ldo=1), "conv3 weights")])
HALO_ACCEPTED = [dict(), dict(conv_pix=32), dict(k_splits=1), dict(conv_Cin=64, K=576, N=64, ldo=72), dict(epi=G.ADD, res1=1, res2=1), dict(epi=G.ADD)]  # what vx_conv3x3_supported still answers 1 for
COLS_REFUSAL_BASE = dict(x=1, om=1, cols=1, B=1, H=5, W=7, C=8, k=3, ldom=27)
COLS_REFUSALS = [(dict(k=2, ldom=12), "kernel 2"), (dict(k=4, ldom=48), "kernel 4"), (dict(k=6, ldom=108), "kernel 6"), (dict(ldom=26), "offset row stride 26"), (dict(k=7, ldom=146), "offset row stride 146"),
                 (dict(C=12), "C = 12"), (dict(k=9, ldom=243), "kernel 9"), (dict(x=0), "bad operands")]

REFUSAL_SCRATCH_BYTES = 1 << 20  # every operand of every accepted base call fits: a refusal that regressed stays in bounds (the extents above that do not fit are refused by their own rule)


def run_refusals(lib, ptr, seen=None):
    """every table entry against the library: returns 0 with its message (before any launch: `ptr` is never dereferenced) -> the number run;
    `seen` collects the messages"""
    import ctypes

    from visioncpp_amd import _lib as L

    def p(v, shift=0):
        return ptr + shift if v else None

    def refused(r, fields, message):
        assert r == 0 and message.encode() in lib.vx_last_error(), (fields, message, lib.vx_last_error())
        if seen is not None:
            seen.append(lib.vx_last_error().decode())

    n = 0
    for fields, message in DEFORM_REFUSALS:
        f = dict(DEFORM_REFUSAL_BASE, **fields)
        d = L.DeformConvArgs()
        d.x, d.w, d.offset, d.out, d.mask = p(f["x"], f["x_shift"]), p(f["w"]), p(f["offset"]), p(f["out"], f["out_shift"]), p(f["mask"])
        d.scale, d.bias = (p(f[k], f["scale_shift"]) for k in ("scale", "bias"))
        for k in ("B", "H", "W", "Cin", "Cout", "k", "pad", "ld_offset", "ld_mask", "mask_mode", "ldo"):
            setattr(d, k, f[k])
        d.mask_scale = 2.0
        refused(lib.vx_deform_conv_f16(ctypes.byref(d), None), fields, message)
        n += 1
    for fields, message in MBCONV_REFUSALS:
        f = dict(MBCONV_REFUSAL_BASE, **fields)
        refused(lib.vx_mbconv_dw_pw_f16(*(p(f[k]) for k in ("h", "w2", "b2", "w3", "b3", "x", "y")), f["B"], f["H"], f["W"], f["C"], f["Cout"], None), fields, message)
        if any(k in fields for k in ("C", "Cout", "W")):
            assert lib.vx_mbconv_dw_pw_supported(f["C"], f["Cout"], f["W"]) == 0
        n += 1
    assert lib.vx_mbconv_dw_pw_supported(256, 64, 64) == 1 and lib.vx_mbconv_dw_pw_supported(256, 64, 192) == 1

    def halo_args(fields):
        f = dict(HALO_REFUSAL_BASE, **fields)
        g = L.GemmArgs()
        for k, v in f.items():
            if k in ("A", "W", "out", "res1", "res2", "lambda_"):
                v = p(v)
            setattr(g, k, v)
        return g

    for fields, message in HALO_REFUSALS:
        g = halo_args(fields)
        refused(lib.vx_conv3x3_f16(ctypes.byref(g), None), fields, message)
        if message in (_SHAPE, "conv_pix", "post_gelu", "window-order", "k_splits", "ld_res1", "a_group", "res2 without res1"):  # the lowering's query answers the same
            assert lib.vx_conv3x3_supported(ctypes.byref(g)) == 0, fields
        n += 1
    for fields in HALO_ACCEPTED:
        g = halo_args(fields)
        assert lib.vx_conv3x3_supported(ctypes.byref(g)) == 1, fields
    for fields, message in COLS_REFUSALS:
        f = dict(COLS_REFUSAL_BASE, **fields)
        refused(lib.vx_bf_deform_cols_f16(p(f["x"]), p(f["om"]), f["ldom"], p(f["cols"]), f["B"], f["H"], f["W"], f["C"], f["k"], None), fields, message)
        n += 1
    return n

"""The case table of vx_dconv3x3_f16's argument space: built the same way by the CPU tests that check the table's completeness
(tests/test_dconv_ref_cpu.py) and by the GPU tests that run it (tests/test_gpu_dconv_matrix.py). A case is a small dict; `materialize` turns it
into the `args` dict of tests/dconv_ref.py (seeded by the case id). The launcher's host-side decisions -- which of its instantiations a call
takes, how many blocks it starts, which tiles a block walks -- are restated here from csrc/kernels_dconv.hip, so that the table can be checked
against them without a device."""
from __future__ import annotations

import zlib

import numpy as np

import dconv_ref as R

F16, RGB, HEAD = R.DC_F16, R.DC_RGB_F32, R.DC_HEAD_F32
GUARD_PIX = 64  # zeroed pixels behind the last image of every output plane / map: a store of a tile's out-of-map lane would land there

# ---- the launcher, restated -------------------------------------------------------------------------------------------------------------

# name -> (COUT, epilogue, AR, STAMP, RES, halo stages, BIL, ONE): every instantiation launch_dconv can select
VARIANTS = {
    "c32": (32, F16, 0, 0, 0, 3, 0, 0), "c32_ar": (32, F16, 1, 0, 0, 3, 0, 0), "c32_stamp": (32, F16, 0, 1, 0, 3, 0, 0),
    "c32_res2": (32, F16, 0, 0, 2, 3, 0, 0), "c32_res4": (32, F16, 0, 0, 4, 2, 0, 0),
    "c64": (64, F16, 0, 0, 0, 2, 0, 0), "c64_ar": (64, F16, 1, 0, 0, 2, 0, 0), "c64_stamp": (64, F16, 0, 1, 0, 2, 0, 0),
    "rgb": (32, RGB, 0, 0, 0, 3, 0, 0), "head": (32, HEAD, 0, 0, 0, 3, 0, 0), "head_one": (32, HEAD, 0, 0, 0, 3, 0, 1),
    "bil": (32, F16, 0, 0, 0, 2, 1, 0), "bil_head": (32, HEAD, 0, 0, 0, 2, 1, 0), "bil_head_one": (32, HEAD, 0, 0, 0, 2, 1, 1),
}


def variant_of(a, res_mode=-1) -> str:
    """launch_dconv's choice for an accepted call; res_mode = VISP_DCONV_RES / vx_dconv_set_resident_mode (-1: default)"""
    epi, cin, cout, bil = a.get("epi", F16), a["cin"], a["cout"], a.get("bil_hs", 0) > 0
    if epi == HEAD:
        return ("bil_head_one" if bil else "head_one") if cin == 32 else ("bil_head" if bil else "head")
    if epi == RGB:
        return "rgb"
    if cout == 32 and bil:
        return "bil"
    if a.get("a_relu"):
        return f"c{cout}_ar"
    if a.get("stamps"):
        return f"c{cout}_stamp"
    if cout == 32:
        if res_mode >= 1 and cin == 64:
            return "c32_res2"
        if (res_mode >= 2 and cin <= 128) or (res_mode < 0 and cin == 128):
            return "c32_res4"
    return f"c{cout}"


def unrolled_period(variant: str) -> int:
    """steps after which the step loop's code positions repeat: 2 slab parities x 3 halo stages, 3 with resident slabs, 2 with two halo stages"""
    _, _, _, _, res, hs, _, _ = VARIANTS[variant]
    return 2 if hs == 2 else (3 if res else 6)


def tile_count(H, W) -> int:
    q, rem = divmod(W, 32)
    main = (q + (1 if rem > 16 else 0)) * ((H + 15) // 16)
    return main + ((H + 31) // 32 if 0 < rem <= 16 else 0)


def grid_blocks(tiles: int, n_cu: int) -> int:
    if tiles > n_cu and n_cu % 8 == 0:
        per_xcd, cu_per_xcd = (tiles + 7) // 8, n_cu // 8
        rounds = (per_xcd + cu_per_xcd - 1) // cu_per_xcd
        return 8 * ((per_xcd + rounds - 1) // rounds)
    return min(tiles, n_cu)


def block_tiles(tiles: int, blocks: int) -> list[list[int]]:
    """the tiles every block walks, in order (the kernel's XCD dealing)"""
    out = []
    per, rem = tiles >> 3, tiles & 7
    for i in range(blocks):
        xcd = i & 7
        lo = xcd * (per + 1) if xcd < rem else rem * (per + 1) + (xcd - rem) * per
        end = lo + per + (1 if xcd < rem else 0)
        step = (blocks - xcd + 7) >> 3
        out.append(list(range(lo + (i >> 3), end, step)))
    return out


# ---- cases ------------------------------------------------------------------------------------------------------------------------------

STREAM_SHAPE = dict(B=5, H=37, W=72)  # 8 tiles per image: 6 of 16x32 (partial bottom row) + 2 of the 32x16 strip; 40 tiles
STREAM_BIL = (19, 37)                 # a supported low-resolution source of a 37 x 72 map
CAPS = (8, 16, 0)                     # 5 tiles per block; stride 2; one tile per block (uncapped)
ALL_CIN = (32, 64, 96, 128, 160, 192)


def _stream():
    forms = {
        "c32": dict(cout=32, layout="planar", act=1, res_mode=0, cins=ALL_CIN),
        "c32_ar": dict(cout=32, layout="nhwc", a_relu=1, act=2, cins=ALL_CIN),
        "c32_res2": dict(cout=32, layout="planar", act=1, res_mode=1, cins=(64,)),
        "c32_res4": dict(cout=32, layout="planar", act=1, res_mode=2, cins=(32, 96, 128)),
        "c64": dict(cout=64, layout="planar", res1=1, res2=1, cins=ALL_CIN),
        "c64_ar": dict(cout=64, layout="nhwc", a_relu=1, act=2, cins=ALL_CIN),
        "rgb": dict(cout=32, layout="planar", epi=RGB, cins=ALL_CIN),
        "head": dict(cout=32, layout="nhwc", epi=HEAD, cins=ALL_CIN[1:]),
        "head_one": dict(cout=32, layout="nhwc", epi=HEAD, cins=(32,)),
        "bil": dict(cout=32, layout="nhwc", bil=STREAM_BIL, res1=1, cins=ALL_CIN),
        "bil_head": dict(cout=32, layout="nhwc", bil=STREAM_BIL, epi=HEAD, cins=ALL_CIN[1:]),
        "bil_head_one": dict(cout=32, layout="nhwc", bil=STREAM_BIL, epi=HEAD, cins=(32,)),
    }
    out = []
    for name, f in forms.items():
        cins = f.pop("cins")
        for cin in cins:
            out.append(dict(STREAM_SHAPE, id=f"{name}-cin{cin}", variant=name, cin=cin, caps=CAPS, **f))
    # the default resident mode (cin = 128 only) next to the forced ones
    out.append(dict(STREAM_SHAPE, id="c32_res4-cin128-default", variant="c32_res4", cin=128, cout=32, layout="planar", act=1, res_mode=-1, caps=CAPS))
    return out


STAMPS = [dict(STREAM_SHAPE, id=f"c{cout}_stamp-cin96", variant=f"c{cout}_stamp", cin=96, cout=cout, layout="planar", act=1, res_mode=0, stamps=1, caps=CAPS)
          for cout in (32, 64)]

RES_FORMS = {"none": (0, 0), "res1": (1, 0), "res1+res2": (1, 1), "res2": (0, 1)}
SCALES = ((1.0, 1.0), (0.2, 0.2), (-0.5, 1.0), (1.0, 0.3))
EPI_SHAPE = dict(B=2, H=19, W=40, cin=32)  # one main column and the strip, two tile rows, one step per tile


def _epilogue():
    out = []
    for cout in (32, 64):
        for act in (0, 1, 2):
            for rname, (r1, r2) in RES_FORMS.items():
                for layout in ("planar", "nhwc"):
                    for s1, s2 in SCALES:
                        out.append(dict(EPI_SHAPE, id=f"c{cout}-act{act}-{rname}-{layout}-s{s1:g}_{s2:g}", cout=cout, act=act, res1=r1, res2=r2, layout=layout, s1=s1, s2=s2))
    for s1 in (0.2, 1.0, -0.5):  # (0.3, an activation and a_relu are refused: the contract table)
        for r2 in (0, 1):
            out.append(dict(B=2, H=19, W=40, cin=96, cout=64, id=f"xres-s{s1:g}-res2_{r2}", layout="planar", x_residual=1, s1=s1, s2=(1.0 if s1 == 1.0 else 0.2), res2=r2))
    return out


def _geometry():
    out = []
    hw = [(1, 1), (15, 17), (16, 16), (17, 15), (31, 33), (32, 32), (33, 31), (1, 48), (33, 49), (16, 1), (17, 32), (32, 48), (15, 31), (31, 16)]
    for i, (H, W) in enumerate(hw):
        cout = (32, 64)[i & 1]
        out.append(dict(id=f"h{H}-w{W}-c{cout}", B=(1, 3)[(i >> 1) & 1], H=H, W=W, cin=64, cout=cout, layout=("planar", "nhwc")[(i >> 1) & 1], act=1, res1=1, s1=0.2))
    for cout in (32, 64):
        for layout in ("planar", "nhwc"):
            for H, W in ((2, 2), (34, 18)):
                out.append(dict(id=f"up2-c{cout}-{layout}-{H}x{W}", B=2, H=H, W=W, cin=64, cout=cout, layout=layout, up2=1, act=1))
    # the interpolating loader at its smallest extents and at a scale on the boundary of vx_dconv_bilinear_supported (BIL_TIGHT: the CPU sweep's set)
    out.append(dict(id="bil-3x3-from-2x2", B=2, H=3, W=3, cin=64, cout=32, layout="nhwc", bil=(2, 2)))
    out.append(dict(id="bil-tight", B=2, H=BIL_TIGHT[0], W=BIL_TIGHT[0], cin=32, cout=32, layout="nhwc", bil=(BIL_TIGHT[1], BIL_TIGHT[1])))
    out.append(dict(id="bil-tight-head", B=1, H=BIL_TIGHT[0], W=BIL_TIGHT[0], cin=32, cout=32, layout="nhwc", bil=(BIL_TIGHT[1], BIL_TIGHT[1]), epi=HEAD))
    return out


BIL_TIGHT = (67, 37)  # (n_out, n_src): accepted, and some 34-row halo needs all 21 source rows (asserted by the CPU sweep)


def _padded():
    return [dict(id=f"cin48-c{cout}-{kind}", B=2, H=20, W=24, cin=64, cin_real=48, cout=cout, layout="nhwc", x_pix=48, nan_guard=1, extremes=(kind == "extremes"), act=0)
            for cout in (32, 64) for kind in ("normal", "extremes")]


GROUPS = {"stream": _stream(), "stamps": STAMPS, "epilogue": _epilogue(), "geometry": _geometry(), "padded": _padded()}


def group(name):
    return GROUPS[name]


def all_cases():
    return [c for g in GROUPS.values() for c in g]


def materialize(c) -> dict:
    rng = np.random.default_rng(zlib.crc32(c["id"].encode()))
    B, H, W, cin, cout = c["B"], c["H"], c["W"], c["cin"], c["cout"]
    epi, planar = c.get("epi", F16), c["layout"] == "planar"
    cin_real = c.get("cin_real", cin)
    up = 1 if c.get("up2") else 0
    Hs, Ws = c["bil"] if c.get("bil") else (H >> up, W >> up)
    a = dict(B=B, H=H, W=W, cin=cin, cout=cout, epi=epi, act=c.get("act", 0), up2=up, a_relu=c.get("a_relu", 0), x_residual=c.get("x_residual", 0),
             s1=c.get("s1", 1.0), s2=c.get("s2", 1.0), stamps=c.get("stamps", 0), bil_hs=0, bil_ws=0)
    if c.get("bil"):
        a["bil_hs"], a["bil_ws"] = c["bil"]

    # the input: the conv reads a channel PREFIX of a wider map (one more plane, resp. 32 more channels per pixel)
    src_pix = B * Hs * Ws
    if planar:
        x = (rng.standard_normal((cin // 32 + 1, src_pix, 32)) * 0.5).astype(np.float16)
        a.update(x=x.reshape(-1), x_off=0, x_plane=src_pix * 32, x_pix=0)
    else:
        xp = c.get("x_pix", cin + 32)
        x = (rng.standard_normal((src_pix, xp)) * 0.5).astype(np.float16)
        if c.get("extremes"):
            x[:, :16] = np.where(rng.random((src_pix, 16)) < 0.5, np.float16(65504), np.float16(-65504))
        flat = x.reshape(-1)
        if c.get("nan_guard"):  # allocated memory behind the map that the descriptor's range check must keep out of the sums
            flat = np.concatenate([flat, np.full(64, np.nan, np.float16)])
        a.update(x=flat, x_off=0, x_plane=32, x_pix=xp)

    cout_real = 3 if epi == RGB else cout
    w = rng.standard_normal((cout_real, cin_real, 3, 3)) / (9 * cin_real if c.get("extremes") else np.sqrt(9 * cin_real))
    a["w"] = R.pack_w(w, cin, cout)
    bias = np.zeros(cout, np.float32)
    bias[:cout_real] = rng.standard_normal(cout_real) * 0.1
    a["bias"] = bias

    pix = B * H * W
    if epi == RGB:
        a.update(out_size=(pix + GUARD_PIX) * 3, out_off=0, out_plane=0, out_pix=0)
    elif epi == HEAD:
        a.update(out_size=pix + GUARD_PIX, out_off=0, out_plane=0, out_pix=0, head_w=np.abs(rng.standard_normal(32) * 0.3).astype(np.float32), head_bias=0.05, head_scale=1.5)
    elif planar:  # planes 1 .. cout/32 of a buffer with one more plane on either side
        plane = (pix + GUARD_PIX) * 32
        a.update(out_size=(cout // 32 + 2) * plane, out_off=plane, out_plane=plane, out_pix=0)
    else:         # channels 16 .. 16 + cout of a map 32 channels wider
        a.update(out_size=(pix + GUARD_PIX) * (cout + 32), out_off=16, out_plane=32, out_pix=cout + 32)
    for which, extra, off in (("res1", 16, 8), ("res2", 64, 24)):
        if not c.get(which):
            continue
        if planar:
            r = (rng.standard_normal((cout // 32, pix, 32)) * 0.5).astype(np.float16)
            a.update({which: r.reshape(-1), which + "_off": 0, which + "_plane": pix * 32, which + "_pix": 0})
        else:
            r = (rng.standard_normal((pix, cout + extra)) * 0.5).astype(np.float16)
            a.update({which: r.reshape(-1), which + "_off": off, which + "_plane": 32, which + "_pix": cout + extra})
    return a

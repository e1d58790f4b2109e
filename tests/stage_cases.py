"""The case tables of the MI-GAN and YOLOv9t stage kernels' argument space -- vx_migan_dwconv_f16 (plain and down kernel),
vx_migan_upsample_f16, vx_migan_torgb, vx_yolo_avgpool2_f16, vx_yolo_spp_f16, vx_yolo_upsample2_f16, vx_yolo_decode -- built the same way by the
CPU tests that check their completeness (tests/test_stage_ref_cpu.py) and by the GPU tests that run them (tests/test_gpu_stage_matrix.py). A case
is a small dict of data only; `materialize` turns it into the `args` dict of tests/stage_ref.py, seeded by the case id. The shapes are the
smallest at which each kernel can still go wrong; the kernels' index arithmetic is restated here from csrc/kernels_migan.hip and
csrc/kernels_yolov9t.hip.

Data kinds: `normal`; `spikes` (bias spikes for the depthwise, large inputs for the upsample: between 1 % and 50 % of the activations lie on
the +-256 clamp in the reference); `negative` (mostly negative pre-activations: the 0.2 slope); `edges` (normal data with +-65504 and f16
subnormals planted; everything stays finite in the reference). vx_yolo_spp_f16: `normal`, `negative` (an all-negative map: a zero from the
padding would win), `lowest` (-65504 everywhere). Every FIR case uses fir_ref.asymmetric_fir except the `symmetric` case of each FIR entry,
which keeps the filter of the trained file. vx_yolo_decode: DFL logits random, one-hot (the expectation is an integer bin, 0 and 15 included)
and all-equal (7.5) by turns; class logits with +-65504 planted; a block of anchors at the head of image 0 whose classes all fail conf = 0.25."""
from __future__ import annotations

import ctypes
import zlib

import numpy as np

import fir_ref
import stage_ref as R

F32 = np.float32
F16 = np.float16

# ---- the kernels' index arithmetic, restated ---------------------------------------------------------------------------------------------------------

DT, DC = 8, 32  # the down kernel's tile of outputs and its channel block


def blocks(n):
    return -(-n // R.BLOCK)


def down_grid(B, H, W, C):
    """(channel blocks, tile rows, tile columns, batch) of migan_dw3x3_agc_down_kernel"""
    return C // DC, -(-(H // 2) // DT), -(-(W // 2) // DT), B


def decode_threads(a):
    """-> (J, image, anchor, item, valid) of every thread of decode_kernel's grid, the padding lanes of the last block included (they act as the last item)"""
    B, S, nc = a["B"], a["S"], a["nc"]
    J, A = 4 + nc // 8, R.n_anchors(S)
    total = B * A * J
    i = np.minimum(np.arange(blocks(total) * R.BLOCK), total - 1)
    return J, i // J // A, i // J % A, i % J, np.arange(i.size) < total


def decode_waves(a):
    """per wave of 64 lanes, from the float64 scores: (candidates, the lanes span two images, the per-lane reservation is taken, candidates in the first
    lane's image, candidates in the other image)"""
    J, b, anchor, item, valid = decode_threads(a)
    s, _ = R.decode_scores(a)
    passing = (s >= float(F32(a["conf"]))).reshape(a["B"], -1, a["nc"] // 8, 8).sum(-1)  # [B, A, groups]
    n = np.where(valid & (item >= 4), passing[b, anchor, np.maximum(item - 4, 0)], 0).reshape(-1, 64)
    bw = b.reshape(-1, 64)
    return n.sum(1), bw[:, 0] != bw[:, -1], ((n > 0) & (bw != bw[:, :1])).any(1), (n * (bw == bw[:, :1])).sum(1), (n * (bw != bw[:, :1])).sum(1)


# ---- the tables -----------------------------------------------------------------------------------------------------------------------------------------

DW_SHAPES = ((1, 2, 2, 64), (2, 3, 5, 64), (2, 5, 7, 64), (1, 4, 6, 128))
DOWN_SHAPES = ((1, 2, 2, 64), (1, 16, 16, 64), (2, 18, 20, 64), (1, 6, 34, 128))
UP_SHAPES = ((1, 1, 1, 8), (2, 2, 3, 8), (1, 5, 9, 24), (2, 4, 4, 16))
TORGB_CASES = (((1, 2, 2, 8), True), ((1, 2, 2, 8), False), ((1, 3, 5, 24), False), ((2, 12, 14, 512), True), ((2, 6, 10, 64), True))
AVGPOOL_CASES = (((1, 2, 2, 8), 8, 0), ((2, 9, 12, 16), 40, 8), ((1, 3, 4, 24), 24, 0))  # (B, H, W, C), pix, c0
SPP_CASES = ((1, 1, 1, 8, 32), (2, 3, 4, 8, 40), (1, 15, 15, 8, 32), (2, 9, 12, 16, 72))
UPSAMPLE2_CASES = (((1, 1, 1, 8), 8, 0, 8, 0), ((2, 3, 5, 16), 40, 8, 24, 8))  # (B, h, w, C), x_pix, c0, y_pix, o0
DECODE_SHAPES = ((1, 32, 8), (2, 64, 16), (3, 96, 8), (1, 64, 80))
CONFS = (0.25, 0.0, 1.5)
KINDS = ("normal", "spikes", "negative", "edges")


def _shape(s):
    return "x".join(str(v) for v in s)


def _dw_cases(entry, shapes, kind_shapes):
    out = [dict(id=f"{entry}-{_shape(s)}-normal", entry=entry, kind="normal", shape=s, fir="asymmetric") for s in shapes]
    out += [dict(id=f"{entry}-{_shape(s)}-{k}", entry=entry, kind=k, shape=s, fir="asymmetric") for s in kind_shapes for k in KINDS[1:]]
    if entry == "dw_down":
        out.append(dict(id=f"{entry}-{_shape(shapes[2])}-symmetric", entry=entry, kind="normal", shape=shapes[2], fir="symmetric"))
    return out


def _up_cases():
    out = [dict(id=f"up-{_shape(s)}-n{n}f{f}-normal", entry="up", kind="normal", shape=s, noise=n, feat=f, fir="asymmetric") for s in UP_SHAPES for n in (1, 0) for f in (1, 0)]
    for s, n, f in ((UP_SHAPES[1], 1, 1), (UP_SHAPES[2], 0, 0)):
        out += [dict(id=f"up-{_shape(s)}-n{n}f{f}-{k}", entry="up", kind=k, shape=s, noise=n, feat=f, fir="asymmetric") for k in KINDS[1:]]
    out.append(dict(id=f"up-{_shape(UP_SHAPES[3])}-n1f1-symmetric", entry="up", kind="normal", shape=UP_SHAPES[3], noise=1, feat=1, fir="symmetric"))
    return out


def _torgb_cases():
    out = [dict(id=f"torgb-{_shape(s)}-prev{int(p)}-normal", entry="torgb", kind="normal", shape=s, prev=int(p), fir="asymmetric") for s, p in TORGB_CASES]
    out.append(dict(id="torgb-2x6x10x64-prev1-edges", entry="torgb", kind="edges", shape=(2, 6, 10, 64), prev=1, fir="asymmetric"))
    out.append(dict(id="torgb-1x3x5x24-prev0-edges", entry="torgb", kind="edges", shape=(1, 3, 5, 24), prev=0, fir="asymmetric"))
    out.append(dict(id="torgb-2x6x10x64-prev1-symmetric", entry="torgb", kind="normal", shape=(2, 6, 10, 64), prev=1, fir="symmetric"))
    return out


def _avgpool_cases():
    return [dict(id=f"avgpool2-{_shape(s)}-pix{pix}-{k}", entry="avgpool2", kind=k, shape=s, pix=pix, c0=c0) for s, pix, c0 in AVGPOOL_CASES for k in ("normal", "edges")]


def _spp_cases():
    out = [dict(id=f"spp-{_shape(s)}-normal", entry="spp", kind="normal", shape=s) for s in SPP_CASES]
    out.append(dict(id=f"spp-{_shape(SPP_CASES[1])}-negative", entry="spp", kind="negative", shape=SPP_CASES[1]))
    out.append(dict(id=f"spp-{_shape(SPP_CASES[2])}-negative", entry="spp", kind="negative", shape=SPP_CASES[2]))
    out.append(dict(id=f"spp-{_shape(SPP_CASES[3])}-lowest", entry="spp", kind="lowest", shape=SPP_CASES[3]))
    return out


def _upsample2_cases():
    return [dict(id=f"upsample2-{_shape(s)}-{k}", entry="upsample2", kind=k, shape=s, x_pix=xp, c0=c0, y_pix=yp, o0=o0) for s, xp, c0, yp, o0 in UPSAMPLE2_CASES for k in ("normal", "edges")]


def _decode_cases():
    out = [dict(id=f"decode-{_shape(s)}-conf{conf:g}", entry="decode", kind=f"conf{conf:g}", shape=s, conf=conf, cand=1) for s in DECODE_SHAPES for conf in CONFS]
    out += [dict(id=f"decode-{_shape(s)}-dense", entry="decode", kind="dense", shape=s, conf=0.25, cand=0) for s in DECODE_SHAPES]
    return out


GROUPS = {"dw": _dw_cases("dw", DW_SHAPES, (DW_SHAPES[2], DW_SHAPES[0])), "dw_down": _dw_cases("dw_down", DOWN_SHAPES, (DOWN_SHAPES[2], DOWN_SHAPES[0])),
          "up": _up_cases(), "torgb": _torgb_cases(), "avgpool2": _avgpool_cases(), "spp": _spp_cases(), "upsample2": _upsample2_cases(), "decode": _decode_cases()}
assert len({c["id"] for g in GROUPS.values() for c in g}) == sum(len(g) for g in GROUPS.values())
assert all(c["entry"] == name for name, g in GROUPS.items() for c in g) and set(GROUPS) == set(R.ENTRIES)


def group(name):
    return GROUPS[name]


def all_cases():
    return [c for g in GROUPS.values() for c in g]


def case(cid):
    return next(c for c in all_cases() if c["id"] == cid)


# ---- materialize --------------------------------------------------------------------------------------------------------------------------------------

def symmetric_fir(rng, C, gain):
    """synth._migan_fir's filter: the [1, 3, 3, 1] outer product, scaled per channel"""
    return fir_ref.perturbed_fir(rng, C, gain)


def fir_of(c, rng, C, gain):
    f = fir_ref.asymmetric_fir(rng, C, gain) if c["fir"] == "asymmetric" else symmetric_fir(rng, C, gain)
    return f.astype(F32)


def plant_edges(v, rng):
    """+-65504 in 6 % of the positions and f16 subnormals of both signs in 10 %; the rest stays"""
    v = np.array(v, F16)
    r = rng.uniform(0, 1, v.shape)
    sign = rng.choice([-1.0, 1.0], v.shape)
    v = np.where(r < 0.06, sign * 65504.0, v)
    sub = rng.integers(1, 1024, v.shape) * 2.0 ** -24 * sign
    return np.where((r >= 0.06) & (r < 0.16), sub, v).astype(F16)


def _dw_args(c, rng):
    B, H, W, C = c["shape"]
    x = rng.standard_normal((B, H, W, C)).astype(F16)
    w = (rng.standard_normal((3, 3, C)) / 3).astype(F16)
    bias = (rng.standard_normal(C) * 0.1).astype(F32)
    if c["kind"] == "spikes":
        ch = np.arange(C)
        bias = np.where(ch % 8 == 1, 300.0 + bias, np.where(ch % 8 == 5, -1200.0 + bias, bias)).astype(F32)
    elif c["kind"] == "negative":
        bias = (-2.0 - np.abs(rng.standard_normal(C))).astype(F32)
    elif c["kind"] == "edges":
        x = plant_edges(x, rng)
    a = dict(B=B, H=H, W=W, C=C, x=x, w=w, bias=bias)
    if c["entry"] == "dw_down":
        a["fir"] = fir_of(c, rng, C, 1.0)
    return a


def _up_args(c, rng):
    B, h, w, C = c["shape"]
    y = rng.standard_normal((B, h, w, C))
    noise = rng.standard_normal((2 * h, 2 * w)) * 0.3 if c["noise"] else None
    feat = rng.standard_normal((B, 2 * h, 2 * w, C)).astype(F16) if c["feat"] else None
    if c["kind"] == "spikes":
        y = y * 300.0
    elif c["kind"] == "negative":
        y = -np.abs(y) - 0.1
        noise = None if noise is None else -np.abs(noise) - 1.0
    y = y.astype(F16)
    if c["kind"] == "edges":
        y = plant_edges(y, rng)
        feat = None if feat is None else np.where(rng.uniform(0, 1, feat.shape) < 0.2, (rng.integers(1, 1024, feat.shape) * 2.0 ** -24), feat).astype(F16)
    return dict(B=B, h=h, w=w, C=C, y=y, fir=fir_of(c, rng, C, 4.0), noise=None if noise is None else noise.astype(F32), feat=feat)


def _torgb_args(c, rng):
    B, H, W, C = c["shape"]
    x = rng.standard_normal((B, H, W, C)).astype(F16)
    if c["kind"] == "edges":
        x = plant_edges(x, rng)
    prev = rng.standard_normal((B, H // 2, W // 2, 3)).astype(F32) if c["prev"] else None
    scale = 16.0 if c["kind"] == "edges" else 1.0  # (sums of a few +-65504 terms stay away from the canary)
    return dict(B=B, H=H, W=W, C=C, x=x, w=(rng.standard_normal((3, C)) / np.sqrt(C) / scale).astype(F32), bias=rng.standard_normal(3).astype(F32), prev=prev,
                fir=fir_of(c, rng, 3, 4.0))


def _decode_args(c, rng):
    B, S, nc = c["shape"]
    A, J = R.n_anchors(S), 4 + nc // 8
    flat = rng.standard_normal((B, A, 64 + nc)) * 2.0
    flat[..., 64:] -= 1.5
    dfl = flat[..., :64].reshape(B, A, 4, 16)
    for b in range(B):
        for an in range(A):
            for side in range(4):
                turn = (an * 4 + side + 3 * b) % 7
                if turn == 0:  # one-hot: bins 0, 15, then by turns; +-30 and the f16 extremes
                    k = (0, 15)[(an // 7) % 2] if an < 14 else (an + side) % 16
                    big = 65504.0 if (an // 7) % 2 else 30.0
                    dfl[b, an, side] = -big
                    dfl[b, an, side, k] = big
                elif turn == 1:
                    dfl[b, an, side] = (an % 5 - 2) * 1.5
    cls = flat[..., 64:]
    r = rng.uniform(0, 1, cls.shape)
    cls[r < 0.01], cls[r > 0.99] = -65504.0, 65504.0
    cls[:, A - 1, 0], cls[:, A - 1, 1] = 65504.0, -65504.0  # the sigmoid saturates to exactly 1 and exactly 0
    quiet = min(A, -(-64 // J) + 1)  # the anchors of a whole wave at the head of image 0: no class reaches conf = 0.25
    cls[0, :quiet] = -4.0 - np.abs(cls[0, :quiet].clip(-8, 8))
    raws, off = [], 0
    for g in R.grids(S):
        raws.append(np.ascontiguousarray(flat[:, off:off + g * g].reshape(B, g, g, 64 + nc)).astype(F16))
        off += g * g
    return dict(B=B, S=S, nc=nc, conf=c["conf"], cand=c["cand"], raws=raws)


def materialize(c) -> dict:
    rng = np.random.default_rng(zlib.crc32(c["id"].encode()))
    e = c["entry"]
    if e in ("dw", "dw_down"):
        return _dw_args(c, rng)
    if e == "up":
        return _up_args(c, rng)
    if e == "torgb":
        return _torgb_args(c, rng)
    if e == "avgpool2":
        B, H, W, C = c["shape"]
        x = rng.standard_normal((B, H, W, c["pix"])).astype(F16)
        if c["kind"] == "edges":
            x = plant_edges(x, rng)
            x[0, 0, 0, c["c0"]], x[0, 0, 1, c["c0"]], x[0, 1, 0, c["c0"]], x[0, 1, 1, c["c0"]] = 65504.0, 65504.0, 65504.0, 65504.0  # the mean is 65504 itself
        return dict(B=B, H=H, W=W, C=C, pix=c["pix"], c0=c["c0"], x=x)
    if e == "spp":
        B, H, W, C, pix = c["shape"]
        x = rng.standard_normal((B, H, W, C))
        x = -np.abs(x) - 0.01 if c["kind"] == "negative" else np.full_like(x, -65504.0) if c["kind"] == "lowest" else np.where(x == 0, 1.0, x)
        buf = np.full((B, H, W, pix), R.CANARY, F16)
        buf[..., :C] = x.astype(F16)
        return dict(B=B, H=H, W=W, C=C, pix=pix, buf=buf)
    if e == "upsample2":
        B, h, w, C = c["shape"]
        x = rng.standard_normal((B, h, w, c["x_pix"])).astype(F16)
        if c["kind"] == "edges":
            x = plant_edges(x, rng)
            x[0, 0, 0, c["c0"]], x[0, 0, 0, c["c0"] + 1] = -0.0, 0.0  # a copy keeps the sign of a zero: the comparison is of bits
        return dict(B=B, h=h, w=w, C=C, x_pix=c["x_pix"], c0=c["c0"], y_pix=c["y_pix"], o0=c["o0"], x=x)
    assert e == "decode"
    return _decode_args(c, rng)


GUARD = R.BLOCK * 8
COUNT_GUARD = 64


# ---- the refusals: (fields changed from an accepted base call, message fragment); nothing here is built to fault -----------------------------------
# A pointer field holds 0 (NULL), k > 0 (region k - 1 of the scratch, 64 KiB each: the operands of a call do not overlap, so a base call, and a
# refusal should it regress, computes on zeros inside the scratch) or -k (2 bytes into region k - 1: misaligned).

REGION = 1 << 16
REFUSAL_SCRATCH_BYTES = 1 << 20
_AL = "must be 16-byte aligned"
DW_BASE = dict(x=1, w=2, bias=3, fir=0, y=5, B=1, H=2, W=2, C=64)
DW_REFUSALS = ([(dict(**{k: 0}), "vx_migan_dwconv_f16: null pointer") for k in ("x", "w", "bias", "y")]
               + [(dict(**{k: -v}), "vx_migan_dwconv_f16: x, w and y " + _AL) for k, v in (("x", 1), ("w", 2), ("y", 5))]
               + [(f, "vx_migan_dwconv_f16: bad extent") for f in (dict(B=0), dict(B=-1), dict(H=1), dict(W=1), dict(H=0))]
               + [(dict(C=C), f"C={C} must be a positive multiple of 64") for C in (0, 32, 96, -64)]
               + [(dict(fir=4, H=3, W=4), "downsample needs an even extent (4x3)"), (dict(fir=4, H=4, W=3), "downsample needs an even extent (3x4)"),
                  (dict(fir=4, B=65536), "batch 65536 too large")])
UP_BASE = dict(y=1, fir=2, noise=3, feat=4, out=5, B=1, h=1, w=1, C=8)
UP_REFUSALS = ([(dict(**{k: 0}), "vx_migan_upsample_f16: null pointer") for k in ("y", "fir", "out")]
               + [(dict(**{k: -v}), "vx_migan_upsample_f16: y, feat and out " + _AL) for k, v in (("y", 1), ("feat", 4), ("out", 5))]
               + [(f, "vx_migan_upsample_f16: bad extent") for f in (dict(B=0), dict(h=0), dict(w=0), dict(h=-1))]
               + [(dict(C=C), f"C={C} must be a positive multiple of 8") for C in (0, 4, 12, -8)])
TORGB_BASE = dict(x=1, w=2, bias=3, prev=4, fir=5, img=6, B=1, H=2, W=2, C=8)
TORGB_REFUSALS = ([(dict(**{k: 0}), "vx_migan_torgb: null pointer") for k in ("x", "w", "bias", "img")]
                  + [(dict(x=-1), "vx_migan_torgb: x " + _AL)]
                  + [(f, "the image path needs its FIR and an even extent") for f in (dict(fir=0), dict(H=3), dict(W=3))]
                  + [(f, "vx_migan_torgb: bad extent") for f in (dict(B=0), dict(H=0), dict(W=0), dict(prev=0, H=-1))]
                  + [(dict(C=C), f"C={C} must be a multiple of 8 in [8, 512]") for C in (0, 4, 12, 520)])
PRE_BASE = dict(img=1, ch=3, mask=2, in4=0, w=3, bias=4, out=5, n=4, C=8)
PRE_REFUSALS = ([(dict(**{k: 0}), "vx_migan_preprocess: null pointer") for k in ("w", "bias", "out")]
                + [(dict(out=-5), "vx_migan_preprocess: out " + _AL)]
                + [(f, "need an f32 input or a 3/4-channel u8 image and a mask") for f in (dict(img=0), dict(mask=0), dict(ch=2), dict(ch=5))]
                + [(f, "vx_migan_preprocess: bad shape") for f in (dict(n=0), dict(n=-1), dict(C=0), dict(C=4))])
AVG_BASE = dict(x=1, x_pix=8, y=2, B=1, H=2, W=2, C=8)
AVG_REFUSALS = [(f, "vx_yolo_avgpool2_f16: bad shape") for f in (dict(x=0), dict(y=0), dict(B=0), dict(H=1), dict(W=1), dict(C=0), dict(C=4), dict(x_pix=0), dict(x_pix=12, C=8),
                                                                dict(x_pix=16, C=24), dict(x=-1), dict(y=-2))]
SPP_BASE = dict(buf=1, pix=32, B=1, H=1, W=1, C=8)
SPP_REFUSALS = [(f, "vx_yolo_spp_f16: bad shape") for f in (dict(buf=0), dict(B=0), dict(H=0), dict(W=0), dict(C=0), dict(C=4), dict(pix=24), dict(pix=36), dict(buf=-1))]
UP2_BASE = dict(x=1, x_pix=8, y=2, y_pix=8, B=1, h=1, w=1, C=8)
UP2_REFUSALS = [(f, "vx_yolo_upsample2_f16: bad shape") for f in (dict(x=0), dict(y=0), dict(B=0), dict(h=0), dict(w=0), dict(C=0), dict(C=4), dict(x_pix=0), dict(y_pix=0),
                                                                 dict(x_pix=12), dict(y_pix=12), dict(x=-1), dict(y=-2))]
DECODE_BASE = dict(raw0=1, raw1=2, raw2=3, boxes=4, scores=5, count=6, idx=7, score=8, B=1, S=32, nc=8, conf=0.25)
DECODE_REFUSALS = ([(dict(**{k: 0}), "vx_yolo_decode: null or misaligned operand") for k in ("raw0", "raw1", "raw2", "boxes", "scores")]
                   + [(dict(**{k: -v}), "vx_yolo_decode: null or misaligned operand") for k, v in (("raw0", 1), ("raw1", 2), ("raw2", 3), ("scores", 5))]
                   + [(f, "vx_yolo_decode: bad shape") for f in (dict(B=0), dict(S=0), dict(S=48), dict(S=-32), dict(nc=0), dict(nc=4))]
                   + [(dict(**{k: 0}), "the candidate list needs count, index and score buffers") for k in ("count", "idx", "score")]
                   + [(dict(count=0, idx=0), "the candidate list needs count, index and score buffers")])
REFUSAL_TABLES = {"dw": DW_REFUSALS, "up": UP_REFUSALS, "torgb": TORGB_REFUSALS, "preprocess": PRE_REFUSALS, "avgpool2": AVG_REFUSALS, "spp": SPP_REFUSALS,
                  "upsample2": UP2_REFUSALS, "decode": DECODE_REFUSALS}
REFUSAL_BASES = {"dw": DW_BASE, "up": UP_BASE, "torgb": TORGB_BASE, "preprocess": PRE_BASE, "avgpool2": AVG_BASE, "spp": SPP_BASE, "upsample2": UP2_BASE, "decode": DECODE_BASE}
EXTRA_BASES = [("dw", dict(DW_BASE, fir=4)), ("up", dict(UP_BASE, noise=0, feat=0)), ("torgb", dict(TORGB_BASE, prev=0, fir=0, H=3, W=5)),
               ("decode", dict(DECODE_BASE, count=0, idx=0, score=0))]  # the other accepted forms of the launchers
# every clause of every VX_REQUIRE of a launcher, in the source's order -> the row of its table that fails that clause and no other
# (tests/test_stage_ref_cpu.py holds the keys to the source text and the rows to the tables)
_A16 = "aligned16({})".format
CLAUSE_ROWS = {
    "dw": {"x": dict(x=0), "w": dict(w=0), "bias": dict(bias=0), "y": dict(y=0), _A16("x"): dict(x=-1), _A16("w"): dict(w=-2), _A16("y"): dict(y=-5), "B > 0": dict(B=0),
           "H >= 2": dict(H=1), "W >= 2": dict(W=1), "C > 0": dict(C=0), "C % 64 == 0": dict(C=32), "H % 2 == 0": dict(fir=4, H=3, W=4), "W % 2 == 0": dict(fir=4, H=4, W=3),
           "B <= 65535": dict(fir=4, B=65536)},
    "up": {"y": dict(y=0), "fir": dict(fir=0), "out": dict(out=0), _A16("y"): dict(y=-1), _A16("feat"): dict(feat=-4), _A16("out"): dict(out=-5), "B > 0": dict(B=0),
           "h > 0": dict(h=0), "w > 0": dict(w=0), "C > 0": dict(C=0), "C % 8 == 0": dict(C=4)},
    "torgb": {"x": dict(x=0), "w": dict(w=0), "bias": dict(bias=0), "img": dict(img=0), _A16("x"): dict(x=-1), "!img_prev": dict(fir=0), "fir": dict(fir=0),
              "H % 2 == 0": dict(H=3), "W % 2 == 0": dict(W=3), "B > 0": dict(B=0), "H > 0": dict(H=0), "W > 0": dict(W=0), "C > 0": dict(C=0), "C % 8 == 0": dict(C=4),
              "C <= 512": dict(C=520)},
    "preprocess": {"w": dict(w=0), "bias": dict(bias=0), "out": dict(out=0), _A16("out"): dict(out=-5), "in4": dict(img=0), "img": dict(img=0), "mask": dict(mask=0),
                   "img_channels == 3": dict(ch=2), "img_channels == 4": dict(ch=5), "n_pixels > 0": dict(n=0), "C > 0": dict(C=0), "C % 8 == 0": dict(C=4)},
    "avgpool2": {"x": dict(x=0), "y": dict(y=0), "B > 0": dict(B=0), "H >= 2": dict(H=1), "W >= 2": dict(W=1), "C > 0": dict(C=0), "C % 8 == 0": dict(C=4),
                 "x_pix >= C": dict(x_pix=16, C=24), "x_pix % 8 == 0": dict(x_pix=12, C=8), _A16("x"): dict(x=-1), _A16("y"): dict(y=-2)},
    "spp": {"buf": dict(buf=0), "B > 0": dict(B=0), "H > 0": dict(H=0), "W > 0": dict(W=0), "C > 0": dict(C=0), "C % 8 == 0": dict(C=4), "pix >= 4 * C": dict(pix=24),
            "pix % 8 == 0": dict(pix=36), _A16("buf"): dict(buf=-1)},
    "upsample2": {"x": dict(x=0), "y": dict(y=0), "B > 0": dict(B=0), "h > 0": dict(h=0), "w > 0": dict(w=0), "C > 0": dict(C=0), "C % 8 == 0": dict(C=4),
                  "x_pix >= C": dict(x_pix=0), "y_pix >= C": dict(y_pix=0), "x_pix % 8 == 0": dict(x_pix=12), "y_pix % 8 == 0": dict(y_pix=12), _A16("x"): dict(x=-1),
                  _A16("y"): dict(y=-2)},
    "decode": {"raw0": dict(raw0=0), "raw1": dict(raw1=0), "raw2": dict(raw2=0), "boxes": dict(boxes=0), "scores": dict(scores=0), _A16("raw0"): dict(raw0=-1),
               _A16("raw1"): dict(raw1=-2), _A16("raw2"): dict(raw2=-3), _A16("scores"): dict(scores=-5), "B > 0": dict(B=0), "S >= 32": dict(S=0), "S % 32 == 0": dict(S=48),
               "nc > 0": dict(nc=0), "nc % 8 == 0": dict(nc=4), "(cand_count != nullptr) == (cand_idx != nullptr)": dict(count=0),
               "(cand_idx != nullptr) == (cand_score != nullptr)": dict(score=0)},
}
N_REFUSALS = sum(len(t) for t in REFUSAL_TABLES.values())
ENTRY_POINT = {"dw": "vx_migan_dwconv_f16", "dw_down": "vx_migan_dwconv_f16/down", "up": "vx_migan_upsample_f16", "torgb": "vx_migan_torgb", "preprocess": "vx_migan_preprocess",
               "avgpool2": "vx_yolo_avgpool2_f16", "spp": "vx_yolo_spp_f16", "upsample2": "vx_yolo_upsample2_f16", "decode": "vx_yolo_decode"}


def call(lib, entry, f, p):
    """one call of launcher `entry` with the fields f; p(field) turns a pointer field into an address or NULL"""
    if entry in ("dw", "dw_down"):
        return lib.vx_migan_dwconv_f16(p(f["x"]), p(f["w"]), p(f["bias"]), p(f["fir"]), p(f["y"]), f["B"], f["H"], f["W"], f["C"], None)
    if entry == "up":
        return lib.vx_migan_upsample_f16(p(f["y"]), p(f["fir"]), p(f["noise"]), p(f["feat"]), p(f["out"]), f["B"], f["h"], f["w"], f["C"], None)
    if entry == "torgb":
        return lib.vx_migan_torgb(p(f["x"]), p(f["w"]), p(f["bias"]), p(f["prev"]), p(f["fir"]), p(f["img"]), f["B"], f["H"], f["W"], f["C"], None)
    if entry == "preprocess":
        return lib.vx_migan_preprocess(p(f["img"]), f["ch"], p(f["mask"]), p(f["in4"]), p(f["w"]), p(f["bias"]), p(f["out"]), f["n"], f["C"], None)
    if entry == "avgpool2":
        return lib.vx_yolo_avgpool2_f16(p(f["x"]), f["x_pix"], p(f["y"]), f["B"], f["H"], f["W"], f["C"], None)
    if entry == "spp":
        return lib.vx_yolo_spp_f16(p(f["buf"]), f["pix"], f["B"], f["H"], f["W"], f["C"], None)
    if entry == "upsample2":
        return lib.vx_yolo_upsample2_f16(p(f["x"]), f["x_pix"], p(f["y"]), f["y_pix"], f["B"], f["h"], f["w"], f["C"], None)
    assert entry == "decode"
    return lib.vx_yolo_decode(p(f["raw0"]), p(f["raw1"]), p(f["raw2"]), f["B"], f["S"], f["nc"], p(f["boxes"]), p(f["scores"]), ctypes.c_float(f["conf"]), p(f["count"]),
                              p(f["idx"]), p(f["score"]), None)


def region(ptr):
    """-> p(flag) of the refusal tables on the scratch at `ptr`"""
    return lambda k: None if k == 0 else ptr + (abs(k) - 1) * REGION + (2 if k < 0 else 0)


def run_refusals(lib, ptr, seen=None):
    """every table entry against the library: returns 0 with its message (before any launch: `ptr` is never dereferenced) -> the number run"""
    n = 0
    for entry, table in REFUSAL_TABLES.items():
        for fields, message in table:
            r = call(lib, entry, dict(REFUSAL_BASES[entry], **fields), region(ptr))
            assert r == 0 and message.encode() in lib.vx_last_error(), (entry, fields, message, lib.vx_last_error())
            if seen is not None:
                seen.append((entry, lib.vx_last_error().decode()))
            n += 1
    return n


def run_base_calls(lib, ptr):
    """the base call of every table, and the launchers' other accepted forms, are accepted (on a scratch of its own: these calls launch)"""
    forms = list(REFUSAL_BASES.items()) + EXTRA_BASES
    for entry, base in forms:
        assert call(lib, entry, base, region(ptr)) == 1, (entry, base, lib.vx_last_error())
    return len(forms)

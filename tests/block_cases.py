"""The argument space of vx_dino_block16_f16 as data: the case table of tests/test_gpu_block_matrix.py and tests/test_block_ref_cpu.py, the
refusal table, and `materialize` (case -> the arguments tests/block_ref.py takes). The smallest shapes that reach each code path; nothing above
M = 400 (the north-star 2 x 1370 shape stays in tests/test_gpu_block.py). Weight sets are built, and packed, once per set."""
from __future__ import annotations

import zlib

import numpy as np

import block_ref as R

D, HID, HEADS = R.D, R.HID, R.HEADS
INSTANCES = {"TTT": (True, True, True), "TTF": (True, True, False), "TFT": (True, False, True), "TFF": (True, False, False),
             "FTF": (False, True, False)}  # (mlp, qkv, tap): the five the launcher can select
ROWS = (1, 15, 16, 17, 113, 127, 128, 129, 272)
PAIRS = ((129, 43), (272, 17), (272, 34), (272, 136), (255, 85), (130, 65), (15, 5))  # image boundaries inside a wave, between waves, between workgroups
Q_SCALES = (0.125, 1.0, 0.03125)
EPSILONS = (1e-6, 1e-5, 1e-2)
ROW_CLASSES = ("ordinary", "small", "big", "offset", "spike", "tiny", "zero")
# the classes along the rows of a call, shifted by 3 from one wave to the next: neighbours of every kind share a wave, every class meets every lane
PATTERN = ("ordinary", "small", "ordinary", "big", "ordinary", "offset", "ordinary", "spike", "tiny", "zero")
SPECIALS = (0.0, 255.0, -255.0, 256.0, -256.0, 300.0, -300.0, -1000.0, -65504.0, -7.0e4, 6e-8, 6.2e-5)
PROBE_M = 48
ATT_NAN_ROWS = 16  # f16 NaN rows behind att: allocated memory that no accepted call may weigh in
X_GUARD_VALUE = 7.25


def row_classes(M):
    if M == 1:
        return ["ordinary"]
    return [PATTERN[(m + 3 * (m // 16)) % len(PATTERN)] for m in range(M)]


# ---- the table ---------------------------------------------------------------------------------------------------------------------------------

def _case(cid, inst, M, T, q_scale=0.125, eps=1e-6, cap=True, wset="dense", data="mixed", **kw):
    return dict(id=cid, inst=inst, M=M, T=T, q_scale=q_scale, eps=eps, cap=cap, wset=wset, data=data, **kw)


def _grid():
    """every instance at every M; with q / k / v on, T = M (one image) and T = 1 (every token its own image) alternate along M, TTF taking the
    opposite choice of TTT and FTF, so both are present at every M; the scalars and cap cycle"""
    out, n = [], 0
    for inst in INSTANCES:
        for i, M in enumerate(ROWS):
            one_image = (i % 2 == 0) != (inst == "TTF")
            T = M if one_image or not INSTANCES[inst][1] else 1
            out.append(_case(f"{inst}-m{M}-t{T}", inst, M, T, Q_SCALES[n % 3], EPSILONS[(n // 3) % 3], cap=n % 2 == 0))
            n += 1
    return out


def _pairs():
    return [_case(f"{inst}-m{M}-t{T}", inst, M, T, cap=inst == "TTT") for M, T in PAIRS for inst in ("TTT", "FTF")]


def _scalars():
    """q_scale x eps on data where eps matters: bo' = 0, so the tiny rows reach LN2 with a variance of about eps (LN1 in the QKV-only instance)"""
    out = [_case(f"TTT-m33-t11-qs{qs}-eps{eps}", "TTT", 33, 11, qs, eps, cap=False, wset="dense-bo0") for qs in Q_SCALES for eps in EPSILONS]
    return out + [_case(f"FTF-m33-t11-eps{eps}", "FTF", 33, 11, 0.125, eps, wset="dense-bo0") for eps in EPSILONS]


def _probes():
    out = [_case(f"probe-hidden-s{s}", "TTT", PROBE_M, 16, wset=f"hidden-s{s}", data="zeros", s=s, b1="sweep", fc2_random_signs=False) for s in range(4)]
    out += [_case(f"probe-hidden-special-s{s}", "TTT", PROBE_M, 16, wset=f"hidden-special-s{s}", data="zeros", s=s, b1="special", fc2_random_signs=False)
            for s in (0, 3)]
    out.append(_case("probe-outproj", "TTT", PROBE_M, 16, wset="outproj", data="integers", exact_cap=True))
    out += [_case(f"probe-qkv-t{T}", "TTT", PROBE_M, T, q_scale=0.03125, wset="qkv-onehot", qkv_probe=True) for T in (16, 12)]
    return out


GROUPS = {"grid": _grid(), "pairs": _pairs(), "scalars": _scalars(), "probes": _probes()}


def group(name):
    return GROUPS[name]


def all_cases():
    return [c for g in GROUPS.values() for c in g]


def dense_cases():
    return [c for c in all_cases() if c["wset"].startswith("dense")]


# ---- weight sets -------------------------------------------------------------------------------------------------------------------------------

def _h(a):
    return np.ascontiguousarray(np.asarray(a).astype(np.float16))


def sweep_b1():
    """1536 points of [-12, 12], each on one unit: ascending along the units, except that the 64 f32-path units (0 .. 31, 1504 .. 1535) trade
    places with every 8th point of [-2, 2] (a dense stretch where the GELU bends), and units 32 / 1503 hold the neighbours of 31's / 1504's values"""
    perm = np.arange(HID)
    def swap(a, b):
        perm[a], perm[b] = perm[b], perm[a]
    for j in range(32):
        swap(j, 640 + 8 * j)
    for j in range(32):
        swap(HID - 32 + j, 644 + 8 * j)
    swap(32, 640 + 8 * 31 + 1)
    swap(HID - 33, 643)
    return np.linspace(-12.0, 12.0, HID)[perm].astype(np.float32), perm


def special_b1(s):
    """every special value on f32-path units and on packed-f16 units of the 384 units case s observes; the rest a sweep of [-6, 6]"""
    lo = 384 * s
    b1 = np.zeros(HID, np.float32)
    b1[lo:lo + 384] = np.linspace(-6.0, 6.0, 384)
    f32_at = lo if s == 0 else HID - 32
    pk_at = lo + 40 if s == 0 else lo + 100
    for at in (f32_at, f32_at + 16, pk_at, pk_at + 150):
        b1[at:at + len(SPECIALS)] = SPECIALS
    return b1


QKV_PERM = (np.arange(3 * D) * 211 + 17) % D  # the channel each q / k / v feature of the one-hot probe reads

_WSETS = {}


def weights(name):
    """-> dict(wo, w1, w2, wqkv f16 (LayerScale folded in), vec_mlp, vec_qkv, vec_tap f32)"""
    if name in _WSETS:
        return _WSETS[name]
    rng = np.random.default_rng(2024)
    r = lambda *s, scale=1.0: rng.standard_normal(s) * scale  # noqa: E731
    lam1, lam2 = 0.1 + r(D, scale=0.01), 0.1 + r(D, scale=0.01)
    wo, bo = _h(lam1[:, None] * _h(r(D, D, scale=D ** -0.5)).astype(np.float64)), lam1 * r(D, scale=0.1)
    g2, b2 = 1 + r(D, scale=0.05), r(D, scale=0.05)
    w1, b1 = _h(r(HID, D, scale=D ** -0.5)), r(HID, scale=0.1)
    w2, bfc2 = _h(lam2[:, None] * _h(r(D, HID, scale=HID ** -0.5)).astype(np.float64)), lam2 * r(D, scale=0.1)
    gn, bn, wqkv, bqkv = 1 + r(D, scale=0.05), r(D, scale=0.05), _h(r(3 * D, D, scale=D ** -0.5)), r(3 * D, scale=0.1)
    gf, bf = 1 + r(D, scale=0.05), r(D, scale=0.05)
    if name == "dense-bo0":
        bo = np.zeros(D)
    elif name.startswith("hidden-"):
        s = int(name[-1])
        g2, b2, bo, bfc2 = np.zeros(D), np.zeros(D), np.zeros(D), np.zeros(D)
        b1 = special_b1(s) if "special" in name else sweep_b1()[0]
        w2 = np.zeros((D, HID), np.float16)
        w2[np.arange(D), np.arange(D) + 384 * s] = 1.0
    elif name == "outproj":
        wo, bo = _h(np.eye(D)), np.zeros(D)
    elif name == "qkv-onehot":
        gn, bn, bqkv = np.ones(D), np.zeros(D), np.zeros(3 * D)
        wqkv = np.zeros((3 * D, D), np.float16)
        wqkv[np.arange(3 * D), QKV_PERM] = 1.0
    else:
        assert name == "dense", name
    f32 = lambda *v: np.ascontiguousarray(np.concatenate(v).astype(np.float32))  # noqa: E731
    w = dict(wo=wo, w1=w1, w2=w2, wqkv=wqkv, vec_mlp=f32(bo, np.zeros(D), g2, b2, b1, bfc2, np.zeros(D)), vec_qkv=f32(gn, bn, bqkv), vec_tap=f32(gf, bf))
    assert w["vec_mlp"].size == 3840 and w["vec_qkv"].size == 1920 and w["vec_tap"].size == 768
    _WSETS[name] = w
    return w


_PACKED = {}


def packed(name, lib):
    """the two slab streams of a weight set through the library's host packers (no device), built once per set"""
    if name not in _PACKED:
        w = weights(name)
        mlp = np.zeros(lib.vx_dino_block_mlp_bytes() // 2, np.uint16)
        qkv = np.zeros(lib.vx_dino_block_qkv_bytes() // 2, np.uint16)
        assert lib.vx_dino_block16_pack_mlp(w["wo"].ctypes.data, w["w1"].ctypes.data, w["w2"].ctypes.data, mlp.ctypes.data) == 1
        assert lib.vx_dino_block16_pack_qkv(w["wqkv"].ctypes.data, qkv.ctypes.data) == 1
        _PACKED[name] = (mlp, qkv)
    return _PACKED[name]


# ---- materialize ------------------------------------------------------------------------------------------------------------------------------

def make_rows(c):
    """-> x f32 [M + guard, 384] (the guard rows hold a value of their own), att f16 [M + ATT_NAN_ROWS, 384] (NaN behind row M - 1)"""
    M = c["M"]
    rng = np.random.default_rng(zlib.crc32(c["id"].encode()))
    x = np.full((M + R.ROW_GUARD, D), X_GUARD_VALUE, np.float32)
    att = np.full((M + ATT_NAN_ROWS, D), np.nan, np.float16)
    if c["data"] == "zeros":
        x[:M], att[:M] = 0, 0
    elif c["data"] == "integers":  # small integers that encode (m, c): exact in f16 and f32, and so is their sum
        m, ch = np.arange(M)[:, None], np.arange(D)[None, :]
        x[:M] = (m * 5 + ch * 11) % 127 - 63
        att[:M] = (m * 7 + ch * 3) % 61 - 30
    else:
        xs = rng.standard_normal((M, D)) * 1.5 + rng.standard_normal((1, D)) * 0.5
        at = rng.standard_normal((M, D))
        for m, cls in enumerate(row_classes(M)):
            if cls == "small":
                xs[m] *= 0.01
            elif cls == "big":
                xs[m] *= 100.0
            elif cls == "offset":
                xs[m] = 30.0 + 0.5 * rng.standard_normal(D)
            elif cls == "spike":  # one channel at +-300 among channels of size 1, as trained DINOv2 streams have
                xs[m] = rng.standard_normal(D)
                xs[m, (37 * m) % D] = 300.0 * (1 - 2 * (m & 1))
            elif cls == "tiny":
                xs[m], at[m] = 1e-3 * rng.standard_normal(D), 0
            elif cls == "zero":
                xs[m], at[m] = 0, 0
        x[:M], att[:M] = xs, at
    return x, att


def materialize(c) -> dict:
    mlp, qkv, tap = INSTANCES[c["inst"]]
    x, att = make_rows(c)
    a = dict(weights(c["wset"]), x=x, att=att if mlp else None, M=c["M"], T=c["T"], H=HEADS, q_scale=c["q_scale"], eps=c["eps"],
             feat=tap, q=qkv, cap=mlp and c["cap"], fc2_random_signs=c.get("fc2_random_signs", True))
    return a


# ---- the refusals: (fields changed from an accepted base call, words of the message); nothing here is built to fault ------------------------

BASE = dict(M=PROBE_M, T=16, H=HEADS, x=1, att=1, w_mlp=1, vec_mlp=1, w_qkv=1, vec_qkv=1, vec_tap=1, feat=1, q=1, k=1, v=1)
QKV_NEEDS = "the QKV half needs"
REFUSALS = (
    [(dict(M=0), "empty problem"), (dict(x=0), "empty problem"), (dict(att=0, q=0), "neither att nor q given"),
     (dict(w_mlp=0), "the MLP half needs w_mlp and vec_mlp"), (dict(vec_mlp=0), "the MLP half needs w_mlp and vec_mlp")]
    + [(dict(**{f: 0}), QKV_NEEDS) for f in ("w_qkv", "vec_qkv", "k", "v", "T", "H")]
    + [(dict(T=7), QKV_NEEDS), (dict(M=47), QKV_NEEDS), (dict(vec_tap=0), "the tap needs vec_tap"),
       (dict(att=0), "a tap without the MLP half"), (dict(M=1398102, T=1), "exceed the 2 GiB buffer range")]
    + [(dict(H=h), f"H = {h}, but the kernel writes embed_dim / 64") for h in (5, 7, 12)])
REFUSAL_SCRATCH_BYTES = 4 << 20  # every operand of the base call fits (the MLP slab stream is 2.6 MB): a refusal that regressed stays in bounds


def run_refusals(lib, ptr):
    """every table entry against the library: returns 0 with its message (before any launch: `ptr` is never dereferenced) -> the number run"""
    import ctypes

    from visioncpp_amd import _lib as L

    for fields, message in REFUSALS:
        f = dict(BASE, **fields)
        a = L.DinoBlockArgs()
        for name in ("x", "att", "w_mlp", "vec_mlp", "w_qkv", "vec_qkv", "vec_tap", "feat", "q", "k", "v"):
            setattr(a, name, ptr if f[name] else None)
        a.M, a.T, a.H, a.q_scale, a.eps = f["M"], f["T"], f["H"], 0.125, 1e-6
        r = lib.vx_dino_block16_f16(ctypes.byref(a), None)
        assert r == 0 and message.encode() in lib.vx_last_error(), (fields, message, lib.vx_last_error())
    return len(REFUSALS)

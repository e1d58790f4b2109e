"""The case table of the attention kernels (tests/test_attn_ref_cpu.py, tests/test_gpu_attn_matrix.py): data only, grouped per entry point, the
smallest shape that reaches each code path. `materialize(case)` turns a case into the argument dict tests/attn_ref.py evaluates. Every (batch,
head, window) has its own random data from default_rng(seed), rounded to f16. q and k have a standard deviation of 1; keys have one length and
query i leans on key i (correlation 0.9) as the two projections of one token do, so whatever T is, every key carries visible weight for some
query (the sensitivity condition of the CPU file: with independent q and k no scale reached it at T = 1370, the allowance's exponential term
being 4e-3 of the largest output). No case holds a query that is masked on every key."""
from __future__ import annotations

import itertools

import numpy as np

LOG2E = 1.4426950408889634
QK_STD = 1.0
QK_RHO = 0.9


def _h(a):
    return np.asarray(a, np.float32).astype(np.float16)


def _qk(rng, q_shape, k_shape, gain=1.0):
    """q and k of standard deviation QK_STD * gain, query i correlated (QK_RHO) with key i mod Tk as the projections of one token are: every key
    then has a query that weighs it visibly, at any T. The token axis is the second to last."""
    k = rng.standard_normal(k_shape).astype(np.float32)
    if k.shape[-1] > 1:   # every key the same length: no key is short enough to lose to all others everywhere (one feature: that would leave two distinct keys)
        k /= np.sqrt((k ** 2).mean(-1, keepdims=True))
    own = np.take(k, np.arange(q_shape[-2]) % k_shape[-2], axis=-2)
    q = QK_RHO * own + np.sqrt(1.0 - QK_RHO ** 2) * rng.standard_normal(q_shape).astype(np.float32)
    return _h(q * (QK_STD * gain)).astype(np.float32), _h(k * (QK_STD * gain)).astype(np.float32)


# ---- vx_attention_f16 ------------------------------------------------------------------------------------------------------------------------
# (T, B, H): the grids (128 queries per block at 4 waves, 256 at 8) include 1, 3, 7, 8, 9, 13, 16, 17 and 23 blocks
ATTENTION_SHAPES = [(1, 1, 1), (31, 1, 3), (32, 7, 1), (33, 1, 8), (63, 3, 3), (64, 13, 1), (65, 2, 8), (127, 17, 1), (128, 23, 1), (129, 1, 1), (255, 1, 2),
                    (256, 1, 3), (257, 1, 3), (511, 1, 2), (512, 2, 2), (513, 2, 2), (769, 1, 1), (1370, 1, 1)]
GRID_SIZES = (1, 3, 7, 8, 9, 13, 16, 17, 23)
ATTENTION = [dict(id=f"T{T}-B{B}-H{H}", entry="attention", T=T, B=B, H=H, data="random", seed=T) for T, B, H in ATTENTION_SHAPES]
ATTENTION += [
    dict(id="spike-T300", entry="attention", T=300, B=1, H=1, data="spike", seed=3),    # a key of tile 3 and one of the last tile beat everything before them
    dict(id="ramp-T449", entry="attention", T=449, B=1, H=1, data="ramp", seed=23),     # scores that rise (or fall, or stay) by 3 per tile
    dict(id="low-T200", entry="attention", T=200, B=1, H=2, data="low", seed=5),        # every score near -40
    dict(id="vmax-T200", entry="attention", T=200, B=1, H=1, data="vmax", seed=9),      # v = +-65504
]
ATTENTION_REFUSALS = [
    (dict(B=0), "empty problem"), (dict(T=0), "empty problem"),
    (dict(q=0), "null operand"), (dict(k=0), "null operand"), (dict(v=0), "null operand"), (dict(out=0), "null operand"),
    (dict(T=1 << 24), "does not fit the buffer descriptor"),
    (dict(B=1 << 16, H=1 << 15, T=1), "too many blocks"),
]


def attention_grid(c, waves):
    return -(-c["T"] // (32 * waves)) * c["B"] * c["H"]


def attention_default_waves(T):
    return 8 if T > 512 else 4   # vx_attention_f16's rule without VISP_ATTN_WAVES


def _attention(c):
    rng = np.random.default_rng(c["seed"])
    B, H, T = c["B"], c["H"], c["T"]
    q, k = _qk(rng, (B, H, T, 64), (B, H, T, 64))
    v = rng.standard_normal((B, H, T, 64)).astype(np.float32)
    if c["data"] == "spike":
        for key in (200, 290):   # a key of tile 3 (a fast-path tile: the fallback must fire and rescale tiles 0-2) and one of the last tile
            k[0, 0, key] = q[0, 0, key] * (12.0 / float((q[0, 0, key] ** 2).sum() * 0.125))  # natural-log score 12 (2^17) for its own query
    elif c["data"] == "ramp":
        ramp = np.arange(T, dtype=np.float32) / 64.0 * 3.0 / LOG2E    # natural-log units through feature 0: +3 per tile in the exp2 domain
        even = np.arange(0, T - 1, 2)   # a rising or falling query cannot see the far end of the ramp: its key doubles the next one, which a flat query owns
        k[..., even, :] = k[..., even + 1, :]
        q[..., 0] = np.array([8.0, 0.0, -8.0, 0.0], np.float32)[np.arange(T) % 4]   # rising, flat, falling, flat
        k[..., 0] = ramp / (8.0 * 0.125)
    elif c["data"] == "low":
        q[..., 0], k[..., 0] = 16.0, -14.0                               # q . k / 8 = -28 -> -40.4 in the exp2 domain
    elif c["data"] == "vmax":
        v = np.where(rng.random(v.shape) < 0.5, np.float32(65504.0), np.float32(-65504.0))
    return dict(entry="attention", q=_h(q * np.float32(0.125 * LOG2E)), k=_h(k), v=_h(v), B=B, H=H, T=T)


# ---- vx_attention_masked_f16 -----------------------------------------------------------------------------------------------------------------
MASKED_T = (1, 7, 32, 33, 49, 64, 65, 96, 100, 128, 129, 144, 257)
_BATCH = [(2, 1), (4, 2), (3, 3)]                      # (B, Bm): Bm in {1, 2, B}
_CONTENT = ["random", "band", "standin", "swin"]


def masked_waves(T):
    """launch_masked's rule: a wave per 32 queries up to two, four from three query blocks on"""
    qb = -(-T // 32)
    return 4 if qb >= 3 else qb


def _masked_cases():
    out = []
    for i, (hd, T) in enumerate(itertools.product((32, 64), MASKED_T)):
        for rot in range(2):   # two rotations per (head_dim, T): every T meets both mask types, both Hm and two contents
            n = 2 * i + rot + (i // len(MASKED_T))
            f32 = (rot + i) % 2
            B, Bm = _BATCH[n % 3]
            content = _CONTENT[n % 4]
            ws = int(round(T ** 0.5))
            if content == "swin" and (ws * ws != T or T < 49):
                content = "standin"
            if content == "band" and T < 96:
                content = "random"
            if content == "swin":
                B, Bm = 4, 2   # an image of 2 x 1 windows, two images
            H = 2 + n % 2
            Hm = H if content == "swin" or (n // 2) % 2 == 0 else 1
            out.append(dict(id=f"hd{hd}-T{T}-{'f32' if f32 else 'f16'}-B{B}-Bm{Bm}-H{H}-Hm{Hm}-{content}", entry="masked", head_dim=hd, T=T, B=B, H=H, Bm=Bm,
                            Hm=Hm, mask_is_f32=f32, content=content, seed=1000 * hd + 2 * T + rot))
    # the paths the issue names that the rotation could miss: head_dim 64 on the aligned vector path with an f16 mask, band and SWIN masks at both head dims
    for hd, T, f32, content in [(64, 96, 0, "band"), (64, 128, 0, "random"), (32, 257, 1, "band"), (64, 257, 0, "band"), (32, 144, 0, "swin"), (64, 64, 1, "swin"),
                                (32, 100, 0, "band"), (64, 129, 1, "band"), (32, 64, 0, "swin"), (64, 49, 0, "swin"), (64, 100, 1, "swin")]:
        B, Bm = (4, 2) if content == "swin" else (2, 2)
        out.append(dict(id=f"hd{hd}-T{T}-{'f32' if f32 else 'f16'}-B{B}-Bm{Bm}-H2-Hm2-{content}-x", entry="masked", head_dim=hd, T=T, B=B, H=2, Bm=Bm, Hm=2,
                        mask_is_f32=f32, content=content, seed=7 * T + hd))
    return out


MASKED = _masked_cases()
MASKED_REFUSALS = [
    (dict(head_dim=48), "head_dim 48 (32 and 64 are built)"),
    (dict(Hm=3), "the mask has 3 heads (1 or 2)"),
    (dict(Bm=3), "the mask's batch 3 does not divide 4"),
    (dict(T=0), "empty problem"), (dict(B=0), "empty problem"), (dict(mask=0), "empty problem"),
]


def swin_bias_and_masks(rng, ws, heads, nwx, nwy):
    """-> table f32 [(2 ws - 1)^2, heads], bias [heads, N, N] (the f16 values of table[index]), masks [nwx * nwy, N, N] of 0 / -inf, from the oracle"""
    from oracle import oracle
    N = ws * ws
    table = (rng.standard_normal(((2 * ws - 1) ** 2, heads)) * 0.5).astype(np.float32)
    idx = oracle.swin_rel_pos_index(ws).reshape(N, N)
    bias = _h(table).astype(np.float32)[idx].transpose(2, 0, 1)
    return table, np.ascontiguousarray(bias), oracle.swin_attention_mask(nwx * ws, nwy * ws, ws)


def _masked(c):
    rng = np.random.default_rng(c["seed"])
    B, H, T, hd, Bm, Hm = c["B"], c["H"], c["T"], c["head_dim"], c["Bm"], c["Hm"]
    q, k = _qk(rng, (B, H, T, hd), (B, H, T, hd))
    v = _h(rng.standard_normal((B, H, T, hd)))
    dtype = np.float32 if c["mask_is_f32"] else np.float16
    mask = rng.standard_normal((Bm, Hm, T, T)).astype(np.float32)
    i, j = np.arange(T)[:, None], np.arange(T)[None, :]
    if c["content"] == "band":      # |i - j| <= 6 live: from T = 96 on, whole 32-key blocks of -inf before and after the live keys of a query
        mask = np.where(np.abs(i - j) <= 6, mask, -np.inf)
    elif c["content"] == "standin":  # the finite stand-ins frameworks write for -inf, on half of the keys; the diagonal and its neighbour stay live
        mask = np.where((rng.random(mask.shape) < 0.5) & (i != j) & ((i + 1) % T != j), np.float32(-1e9 if c["mask_is_f32"] else -1e4), mask)
    elif c["content"] == "swin":     # relative position bias + shift mask of an image of 2 x 1 windows
        ws = int(round(T ** 0.5))
        _, bias, masks = swin_bias_and_masks(rng, ws, Hm, 2, 1)
        assert Bm == 2
        mask = bias[None] + masks[:, None]
    scale = np.float32(LOG2E / np.sqrt(hd))
    return dict(entry="masked", q=_h(q * scale), k=_h(k), v=v, mask=np.ascontiguousarray(mask.astype(dtype)), B=B, H=H, T=T, head_dim=hd, Hm=Hm, Bm=Bm,
                mask_is_f32=c["mask_is_f32"])


# ---- vx_window_attention_f16 / vx_window_attention_masked_f16 ----------------------------------------------------------------------------------
WINDOW_N = (1, 16, 32, 33, 49, 64, 65, 100, 128, 129, 144, 196, 224, 225, 256)   # every QB of {1, 2, 4, 7, 8} and both edges of each
WINDOW = [dict(id=f"N{N}-h{(1, 3)[i % 2]}-w{1 + i % 5}", entry="window", N=N, heads=(1, 3)[i % 2], n_windows=1 + i % 5, ws=0, nwx=0, nwy=0, seed=N)
          for i, N in enumerate(WINDOW_N)]
SHIFT_WS = (4, 7, 8, 10, 12, 14, 16)
SHIFTED = [dict(id=f"ws{ws}-{nwx}x{nwy}-h{(1, 3)[(i + g) % 2]}", entry="window", N=ws * ws, heads=(1, 3)[(i + g) % 2], n_windows=2 * nwx * nwy, ws=ws, nwx=nwx,
                nwy=nwy, seed=100 * ws + nwx)
           for i, ws in enumerate(SHIFT_WS) for g, (nwx, nwy) in enumerate([(1, 1), (3, 1), (2, 3)])]
WINDOW_REFUSALS = [
    (dict(N=0), "0 tokens per window (at most 256)"),
    (dict(N=257), "257 tokens per window (at most 256)"),
    (dict(n_windows=5, nwx=2, nwy=2), "5 windows are not whole images of 2x2"),
    (dict(nwx=2, nwy=0), "windows are not whole images of 2x0"),
]


def window_qb(N):
    """query_blocks(): the instantiated block shapes"""
    return next(qb for qb in (1, 2, 4, 7, 8) if N <= 32 * qb)


def _window(c):
    rng = np.random.default_rng(c["seed"])
    N, heads, n_win = c["N"], c["heads"], c["n_windows"]
    qkv = rng.standard_normal((n_win, N, heads, 3, 32)).astype(np.float32)
    q, k = _qk(rng, (n_win, heads, N, 32), (n_win, heads, N, 32))
    qkv[..., 0, :], qkv[..., 1, :] = q.transpose(0, 2, 1, 3), k.transpose(0, 2, 1, 3)
    qkv = qkv.reshape(n_win * N, heads, 3, 32)
    a = dict(entry="window", qkv=_h(qkv), n_windows=n_win, N=N, heads=heads, nwx=c["nwx"], nwy=c["nwy"], ws=c["ws"], table=None, mask=None)
    if c["ws"]:
        a["table"], a["bias"], a["mask"] = swin_bias_and_masks(rng, c["ws"], heads, c["nwx"], c["nwy"])
    else:
        bias = _h(rng.standard_normal((heads, N, N)) * 0.5).astype(np.float32)
        a["bias"] = np.where((rng.random(bias.shape) < 0.1) & ~np.eye(N, dtype=bool), np.float32(-np.inf), bias)   # some -inf entries, never the diagonal
    return a


# ---- vx_small_attention_f16 --------------------------------------------------------------------------------------------------------------------
SMALL_SHAPES = [(1, 1), (255, 16), (256, 16), (256, 17), (3, 257), (7, 4096), (300, 7)]
SMALL_HD = (1, 4, 8, 16, 32)
SMALL = [dict(id=f"Nq{nq}-Nk{nk}-hd{SMALL_HD[i % 5]}-h{(1, 3)[i % 2]}", entry="small", Nq=nq, Nk=nk, hd=SMALL_HD[i % 5], heads=(1, 3)[i % 2], gain=1.0, seed=nq + nk)
         for i, (nq, nk) in enumerate(SMALL_SHAPES)]
# every head_dim on both kernels (few keys: Nk <= 16 and Nq >= 256), and one with operands x 3: peaked rows
SMALL += [dict(id=f"Nq{nq}-Nk{nk}-hd{hd}-h{heads}", entry="small", Nq=nq, Nk=nk, hd=hd, heads=heads, gain=1.0, seed=3 * (nq + nk) + hd)
          for hd in SMALL_HD for nq, nk, heads in ((256, 16, 3), (100, 17, 1))]
SMALL += [dict(id="Nq64-Nk300-hd32-h3-x3", entry="small", Nq=64, Nk=300, hd=32, heads=3, gain=3.0, seed=77)]
SMALL_REFUSALS = [
    (dict(Nk=4097), "at most 4096 keys, head_dim a power of two <= 32 (Nk = 4097, hd = 8)"),
    (dict(hd=0), "(Nk = 16, hd = 0)"), (dict(hd=3), "(Nk = 16, hd = 3)"), (dict(hd=64), "(Nk = 16, hd = 64)"),
    (dict(Nq=0), "bad operands"),
]


def small_few_keys(c):
    """the dispatcher's rule: the one-thread-per-query kernel"""
    return c["Nk"] <= 16 and c["Nq"] >= 256


def _small(c):
    rng = np.random.default_rng(c["seed"])
    Nq, Nk, C = c["Nq"], c["Nk"], c["heads"] * c["hd"]
    g = np.float32(c["gain"])
    hq, hk = _qk(rng, (c["heads"], Nq, c["hd"]), (c["heads"], Nk, c["hd"]), g)
    q, k = (np.ascontiguousarray(x.transpose(1, 0, 2)).reshape(-1, C) for x in (hq, hk))
    return dict(entry="small", q=_h(q), k=_h(k), v=_h(rng.standard_normal((Nk, C)) * g),
                Nq=Nq, Nk=Nk, heads=c["heads"], hd=c["hd"])


GROUPS = {"attention": ATTENTION, "masked": MASKED, "window": WINDOW, "shifted": SHIFTED, "small": SMALL}
ALL = [c for g in GROUPS.values() for c in g]
_MAKE = {"attention": _attention, "masked": _masked, "window": _window, "small": _small}


def group(name):
    return GROUPS[name]


def materialize(case):
    return _MAKE[case["entry"]](case)

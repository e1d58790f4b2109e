"""The case table of the attention kernels (tests/test_attn_ref_cpu.py, tests/test_gpu_attn_matrix.py): data only, grouped per entry point, the
smallest shape that reaches each code path. `materialize(case)` turns a case into the argument dict tests/attn_ref.py evaluates. Every (batch,
head, window) has its own random data from default_rng(seed), rounded to f16. q and k have a standard deviation of 1; keys have one length and
query i leans on key i (correlation 0.9) as the two projections of one token do, so whatever T is, every key carries visible weight for some
query (the sensitivity condition of the CPU file: with independent q and k no scale reached it at T = 1370, the allowance's exponential term
being 4e-3 of the largest output). No case holds a query that is masked on every key. The `cross` group has fewer queries than keys in places:
_cross says who owns which key there."""
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


# ---- vx_attention_cross_f16 / vx_attention_cross_step_f16 --------------------------------------------------------------------------------------
CROSS_HD = (16, 32, 64)
CROSS_TQ = (1, 31, 32, 33, 64, 65, 96, 97, 128, 129, 257)     # NW 1, 2 and 4, the idle fourth wave (65 .. 96), several blocks, a last block with one live wave
CROSS_TK = (1, 2, 31, 32, 33, 63, 64, 65, 100, 255)           # one part each
CROSS_LONG = [(33, 256), (33, 300), (65, 256), (65, 300)]     # many keys, too many queries to split
CROSS_SPLIT_TQ = (1, 7, 31, 32)
CROSS_SPLIT_TK = (256, 257, 300, 383, 384, 385)               # 2, 3 and 4 parts; a last part of one key (257, 385), a full one (256, 384)
CROSS_FEW = [(300, 1), (513, 7), (300, 32), (513, 1), (300, 7), (513, 32)]   # few keys, many queries: (Tq, Tk), rotated over the head dims


def cross_waves(Tq):
    """launch_cross's rule: a wave per 32 queries up to two, four from three query blocks on"""
    qb = -(-Tq // 32)
    return 4 if qb >= 3 else qb


def cross_parts(Tq, Tk):
    """cx_parts: at most 32 queries and at least 256 keys cut the keys into parts of 128"""
    return -(-Tk // 128) if Tq <= 32 and Tk >= 256 else 1


def cross_partial_bytes(B, H, Tq, Tk, hd):
    """vx_attention_cross_partial_bytes: [B * H][parts][32][hd + 2] floats, nothing for one part"""
    parts = cross_parts(Tq, Tk)
    return B * H * parts * 32 * (hd + 2) * 4 if parts > 1 else 0


def cross_idle_form(Tq):
    """how a block of four waves comes to hold a wave without queries: 'short' (65 .. 96 queries: the fourth wave of the only block), 'last' (the last of
    several blocks has fewer than 97 queries), None"""
    if cross_waves(Tq) != 4 or (Tq - 1) % 128 >= 96:
        return None
    return "short" if Tq <= 128 else "last"


def cross_edge_keys(Tq, Tk):
    """where a defect of the key loop can sit: the first and last key of every 32-key block, of every 128-key part of a split, and key Tk - 1"""
    edge = {Tk - 1}
    for step in (32,) + ((128,) if cross_parts(Tq, Tk) > 1 else ()):
        for k0 in range(0, Tk, step):
            edge |= {k0, min(k0 + step, Tk) - 1}
    return sorted(edge)


def _cross_cases():
    out = []

    def add(hd, Tq, Tk, data="random", mul=1.0, min_bh=1):
        n = len(out)
        B = 1 + n % 3
        H = 2 + n % 2
        if Tq < Tk and data in ("random", "low", "vmax"):   # enough queries over the (b, h) problems to own every edge key once: see _cross
            min_bh = max(min_bh, -(-len(cross_edge_keys(Tq, Tk)) // Tq))
        H = max(H, -(-min_bh // B))
        scale = {0.0: "-s0", 1.0: ""}.get(mul, f"-sx{mul}")
        out.append(dict(id=f"hd{hd}-Tq{Tq}-Tk{Tk}-B{B}-H{H}{scale}{'' if data == 'random' else '-' + data}", entry="cross", hd=hd, Tq=Tq, Tk=Tk, B=B, H=H,
                        mul=mul, data=data, seed=100000 * hd + 300 * Tq + Tk))

    for hi, hd in enumerate(CROSS_HD):
        for i, Tq in enumerate(CROSS_TQ):   # a rotation, not the product: every Tq and every Tk at every head_dim
            add(hd, Tq, CROSS_TK[(i + 3 * hi) % len(CROSS_TK)])
        for Tq, Tk in CROSS_LONG:
            add(hd, Tq, Tk)
        for j, Tk in enumerate(CROSS_SPLIT_TK):
            add(hd, CROSS_SPLIT_TQ[(j + hi) % len(CROSS_SPLIT_TQ)], Tk, min_bh=4 if j == 2 else 1)
    for i, (Tq, Tk) in enumerate(CROSS_FEW):
        add(CROSS_HD[i % 3], Tq, Tk)
    # scale 0: every P is 1, the output is the mean of v
    for hd, Tq, Tk in [(16, 97, 31), (32, 33, 33), (64, 129, 2), (32, 1, 7)]:
        add(hd, Tq, Tk, mul=0.0)
    # another positive scale per head_dim, one of them split
    for hd, Tq, Tk, mul in [(16, 65, 64, 1.7), (32, 7, 300, 0.6), (64, 128, 100, 1.7)]:
        add(hd, Tq, Tk, mul=mul)
    # the data kinds of _attention, each with one part and split
    for hd, Tq, Tk, data in [(32, 100, 100, "spike"), (16, 65, 255, "ramp"), (64, 33, 100, "low"), (32, 97, 65, "vmax"),
                             (16, 7, 300, "spike"), (64, 31, 385, "ramp"), (32, 7, 257, "low"), (16, 32, 384, "vmax"), (32, 7, 300, "cliff")]:
        add(hd, Tq, Tk, data=data)
    return out


CROSS = _cross_cases()
_PB = cross_partial_bytes(1, 2, 7, 300, 16)
_NOTHING, _ALIGN, _SPLIT = "empty problem", "q, k, v must be 16-byte aligned, out 8-byte aligned", "7 queries on 300 keys split the keys into 3 parts and need"
# against a valid base call (tests/test_gpu_attn_matrix.py); "ptr+n": the scratch buffer's address plus n bytes; step None: vx_attention_cross_f16
CROSS_REFUSALS = [
    (dict(head_dim=48), "head_dim 48 (16, 32 and 64 are built)"),
    (dict(q=0), _NOTHING), (dict(k=0), _NOTHING), (dict(v=0), _NOTHING), (dict(out=0), _NOTHING),
    (dict(B=0), _NOTHING), (dict(H=0), _NOTHING), (dict(Tq=0), _NOTHING), (dict(Tk=0), _NOTHING),
    (dict(q="ptr+8"), _ALIGN), (dict(k="ptr+8"), _ALIGN), (dict(v="ptr+8"), _ALIGN), (dict(out="ptr+4"), _ALIGN),
    (dict(Tk=300, partial=0), f"{_SPLIT} {_PB} bytes of partial results (vx_attention_cross_partial_bytes), got 0"),
    (dict(Tk=300, partial_bytes=_PB - 1), f"{_SPLIT} {_PB} bytes of partial results (vx_attention_cross_partial_bytes), got {_PB - 1}"),
    (dict(Tk=300, partial="ptr+2"), _SPLIT),
    (dict(B=1 << 16, H=1 << 15, Tq=1, Tk=1), "too many blocks"),
    (dict(step=0), "vx_attention_cross_step_f16: step 0"), (dict(step=3), "vx_attention_cross_step_f16: step 3"),
]


def _cross(c):
    """Random data as _qk makes it: keys of one length, a query that leans on "its" key. With Tq >= Tk query i owns key i mod Tk. With fewer queries than
    keys the queries of the successive (b, h) problems own successive keys of cross_edge_keys: a defect at a key position is the same in every (b, h), so
    it is enough that every edge key is owned in one of them (the case's H is chosen so that B * H * Tq reaches the edge set)."""
    rng = np.random.default_rng(c["seed"])
    B, H, Tq, Tk, hd = c["B"], c["H"], c["Tq"], c["Tk"], c["hd"]
    scale = np.float32(c["mul"] / np.sqrt(hd))
    k = rng.standard_normal((B, H, Tk, hd)).astype(np.float32)
    k /= np.sqrt((k ** 2).mean(-1, keepdims=True))
    if Tq >= Tk:
        own = np.broadcast_to(np.arange(Tq) % Tk, (B, H, Tq))
    else:
        edge = np.array(cross_edge_keys(Tq, Tk))
        own = edge[np.arange(B * H * Tq) % len(edge)].reshape(B, H, Tq)
    q = QK_RHO * np.take_along_axis(k, own[..., None], axis=2) + np.sqrt(1.0 - QK_RHO ** 2) * rng.standard_normal((B, H, Tq, hd)).astype(np.float32)
    q, k = _h(q * QK_STD).astype(np.float32), _h(k * QK_STD).astype(np.float32)
    v = rng.standard_normal((B, H, Tk, hd)).astype(np.float32)
    if c["data"] in ("spike", "cliff"):
        # a key of a late 32-key block and one of the last block (in a split: of the last part) beat everything before them for their query: natural-log score
        # 12 (the running maximum jumps by 17 in the exp2 domain, the earlier parts' weights are 2^-17), or for "cliff" 112: every earlier P and part weight is 0
        peak = 12.0 if c["data"] == "spike" else 112.0
        for key in (2 * Tk // 3, Tk - 10):
            qo = q[0, 0, key % Tq]
            k[0, 0, key] = qo * (peak / float((qo ** 2).sum() * scale))
    elif c["data"] == "ramp":   # +3 per 32-key block in the exp2 domain through feature 0, for a rising, a flat and a falling query
        q[..., 0] = np.array([8.0, 0.0, -8.0, 0.0], np.float32)[np.arange(Tq) % 4]
        k[..., 0] = (np.arange(Tk, dtype=np.float32) / 32.0 * 3.0 / LOG2E) / (8.0 * scale)
    elif c["data"] == "low":    # scale * q . k near -28 -> -40.4 in the exp2 domain
        q[..., 0], k[..., 0] = 16.0, -28.0 / (16.0 * scale)
    elif c["data"] == "vmax":
        v = np.where(rng.random(v.shape) < 0.5, np.float32(65504.0), np.float32(-65504.0))
    tok = lambda x: np.ascontiguousarray(_h(x).transpose(0, 2, 1, 3))  # noqa: E731  [B, T, H, hd]: token-major rows, as the launcher takes them
    return dict(entry="cross", q=tok(q), k=tok(k), v=tok(v), B=B, H=H, Tq=Tq, Tk=Tk, head_dim=hd, scale=float(scale))


GROUPS = {"attention": ATTENTION, "masked": MASKED, "window": WINDOW, "shifted": SHIFTED, "small": SMALL, "cross": CROSS}
ALL = [c for g in GROUPS.values() for c in g]
_MAKE = {"attention": _attention, "masked": _masked, "window": _window, "small": _small, "cross": _cross}


def group(name):
    return GROUPS[name]


def materialize(case):
    return _MAKE[case["entry"]](case)

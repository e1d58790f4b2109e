"""-m gpu: the graph layer's window ops on the device (csrc/kernels_attn_mask.hip, the roll / pad kernels of kernels_graph.hip, their
lowering) against float64 numpy on f16-rounded operands (tests/graph_window_ref.py), then the SWIN encoder built through
vision.cpp_amd/graph.py::swin_encode against the CPU oracle's restatement of src/visp/arch/swin.cpp, block by block."""
import functools
import itertools
import math

import numpy as np
import pytest

import graph_window_ref as R
from oracle import oracle
from visioncpp_amd import _lib as L
from visioncpp_amd import graph as G
from visioncpp_amd import synth, vision

pytestmark = pytest.mark.gpu

from gpu_util import api, dev, empty, release, sync  # noqa: E402

# ATTENTION_MASKED against float64. The floor of the comparison -- the float64 reference against itself with its output rounded to f16, operands f16
# already -- measures 3.9e-4, 2.8e-4, 3.0e-4 and 4.0e-4 on the four cases below (2^-11 = 4.9e-4 at most: one rounding of the largest output);
# x 4 for the different accumulation order of P V (and the f16 rounding of the scaled q and of P) is 1.6e-3, so the bound is the 4e-3 the
# existing attention tests use on the same output type: max(4 * floor, 4e-3) = 4e-3.
ATTN_FLOOR_MEASURED = 4.0e-4
ATTN_BOUND = max(4 * ATTN_FLOOR_MEASURED, 4e-3)


@pytest.fixture(scope="module")
def device():
    assert api().vx_device_count() > 0, "no HIP device visible: the product path has no CPU fallback"
    return vision.Device.init(vision.Backend.gpu)


@pytest.fixture(autouse=True)
def _release_buffers():
    yield
    release()


def _i64(v):
    import ctypes as C
    return (C.c_int64 * 4)(*v)


# ---- glue ops: pure data movement, bit for bit ---------------------------------------------------------------------------------

MOVING_AXES = [p for p in itertools.permutations(range(4)) if p[0] != 0]  # every axis order that moves ne[0]
SHIFTS = [(0, -3, -3, 0), (8, 2, 0, 1), (-16, 0, 5, -1), (5, -7, 9, 3), (-31, 11, -2, 0)]  # negative, wrapping, whole 8-groups and odd on ne[0]
PADS = [(0, 2, 3, 0), (8, 0, 1, 1), (3, 1, 0, 0), (16, 4, 2, 2)]


@pytest.mark.parametrize("ne", [(24, 5, 7, 2), (30, 5, 3, 1)])  # 24: 16-byte lanes; 30: the scalar tail path
def test_permute_roll_pad_on_activations_are_exact(device, ne):
    rng = np.random.default_rng(ne[0])
    x = rng.standard_normal(ne[::-1]).astype(np.float16)
    g = G.Graph(device)
    m = G.ModelRef(g)
    xi = g.input(ne, G.F16)
    want = {}
    for axes in MOVING_AXES:
        want[g.output(G.permute(m, xi, *axes), f"permute{axes}")] = R.permute(x, axes)
    for s in SHIFTS:
        want[g.output(G.roll(m, xi, *s), f"roll{s}")] = R.roll(x, s)
    for p in PADS:
        want[g.output(G.pad(m, xi, *p), f"pad{p}")] = R.pad(x, p)
    chain = G.pad(m, G.roll(m, G.cont(m, G.permute(m, xi, 1, 0, 2, 3)), 2, -1, 0, 0), 1, 0, 0, 1)  # cont behind permute stays a view
    want[g.output(chain, "chain")] = R.pad(R.roll(R.permute(x, (1, 0, 2, 3)), (2, -1, 0, 0)), (1, 0, 0, 1))
    g.allocate()
    assert not [l for l in g.describe().splitlines() if l.startswith("cont")]
    g.set(xi, x)
    g.compute()
    for t, w in want.items():
        got = g.get(t)
        assert got.shape == w.shape, t
        np.testing.assert_array_equal(got.astype(np.float16), w, err_msg=str(t))


@pytest.mark.parametrize("ne,shift,padto", [((24, 5, 7, 2), (8, -2, 3, 1), (32, 5, 9, 2)), ((30, 5, 3, 1), (-7, 1, 0, 0), (31, 7, 3, 2))])
def test_roll_and_pad_launchers_directly(ne, shift, padto):
    rng = np.random.default_rng(5)
    x = rng.standard_normal(ne[::-1]).astype(np.float16)
    y = empty(x.size * 2)
    L.vx_check(api().vx_roll_f16(dev(x).ptr, y.ptr, _i64(ne), _i64(shift), None))
    sync()
    np.testing.assert_array_equal(y.to_numpy(np.float16, x.shape), R.roll(x, shift))
    want = R.pad(x, tuple(p - n for p, n in zip(padto, ne)))
    z = empty(want.size * 2, zero=False)
    L.vx_check(api().vx_pad_f16(dev(x).ptr, z.ptr, _i64(ne), _i64(padto), None))
    sync()
    np.testing.assert_array_equal(z.to_numpy(np.float16, want.shape), want)
    assert api().vx_pad_f16(dev(x).ptr, z.ptr, _i64(padto), _i64(ne), None) == 0 and b"shrinks" in api().vx_last_error()


# ---- ATTENTION_MASKED ----------------------------------------------------------------------------------------------------------------

def _shift_mask_2x2():
    return G.swin_attention_mask(14, 14, 7)  # [4, 49, 49]: three of the four windows carry -inf entries


def _band(T, half):
    i = np.arange(T)
    return np.where(np.abs(i[:, None] - i[None, :]) <= half, 0.0, -np.inf)  # [T_q, T_k]; query 45 of 50 has keys 0..31 all masked


@functools.lru_cache(maxsize=None)
def _case(name):
    """(hd, heads, T, B, mask [Bm, Hm, T, T] float64, mask kind, q, k, v [B, T, H, hd] as the f16 values, scale, float64 reference)."""
    hd, heads, T, B, kind = {"swin_bias_plus_shift": (32, 3, 49, 8, "constant"), "f32_activation": (32, 1, 49, 2, "f32"),
                             "hd64_broadcast_band": (64, 2, 50, 2, "constant"), "window12_f16": (32, 2, 144, 3, "f16")}[name]
    rng = np.random.default_rng(len(name))
    q, k, v = (R.f16(rng.standard_normal((B, T, heads, hd)) * 0.8) for _ in range(3))
    if name == "swin_bias_plus_shift":
        mask = R.f16(rng.standard_normal((1, heads, T, T)) * 0.7) + _shift_mask_2x2()[:, None]  # [4, 3, 49, 49], Bm = 4 < B
    elif name == "f32_activation":
        mask = (rng.standard_normal((2, 1, T, T)) * 1.5).astype(np.float32).astype(np.float64)
    elif name == "hd64_broadcast_band":
        mask = _band(T, 5)[None, None]
    else:
        mask = R.f16(rng.standard_normal((3, heads, T, T)) * 2.0)
    scale = 1.0 / math.sqrt(hd)
    return hd, heads, T, B, mask, kind, q, k, v, scale, R.attention_masked(q, k, v, mask, scale)


CASES = ["swin_bias_plus_shift", "f32_activation", "hd64_broadcast_band", "window12_f16"]


def test_masks_keep_every_query_alive_and_mask_whole_key_blocks():
    """On the CPU side of the GPU file: no query row of any case is fully masked (such a row is unspecified), every row of the shift mask
    keeps its own key, and the cases do hold what they are there for: queries with a whole 32-key block at -inf."""
    sm = _shift_mask_2x2()
    assert (sm[:, np.arange(49), np.arange(49)] == 0).all() and [int(np.isneginf(w).any()) for w in sm] == [0, 1, 1, 1]
    blocks_masked = 0
    for name in CASES:
        mask = _case(name)[4]
        assert not np.isneginf(mask).all(-1).any(), name
        blocks_masked += int(np.isneginf(mask[..., :32]).all(-1).any())
    assert blocks_masked >= 2  # the shift mask and the band
    assert np.isneginf(_band(50, 5)[45, :32]).all()
    floors = [R.f16_floor(*[_case(n)[i] for i in (6, 7, 8, 4, 9)]) for n in CASES]
    print("f16 floors of the references:", floors)
    assert max(floors) <= ATTN_FLOOR_MEASURED * 1.01, floors


@pytest.mark.parametrize("name", CASES)
def test_attention_masked_node_against_float64(device, name):
    hd, heads, T, B, mask, kind, q, k, v, scale, want = _case(name)
    assert not np.isneginf(mask).all(-1).any()
    g = G.Graph(device)
    m = G.ModelRef(g)
    qi, ki, vi = (g.input((hd, heads, T, B), G.F16, n) for n in "qkv")
    if kind == "constant":
        mt = g.add_weight("mask", mask.astype(np.float32), G.F16)
    else:
        mt = g.input(mask.shape[::-1], G.F32 if kind == "f32" else G.F16, "mask")
    out = g.output(g.op(G.OP_ATTENTION_MASKED, [qi, ki, vi, mt], fparams=[scale]), "out")
    g.allocate()
    att = [l for l in g.describe().splitlines() if l.startswith("attention")]
    assert len(att) == 1 and f"hd={hd}" in att[0] and f"mask=[{mask.shape[1]}, {mask.shape[0]}]" in att[0] and att[0].endswith("(constant)" if kind == "constant" else kind)
    for t, a in ((qi, q), (ki, k), (vi, v)):
        g.set(t, a)
    if kind != "constant":
        g.set(mt, mask)
    g.compute()
    got = g.get(out)
    assert np.isfinite(got).all()
    err = R.rel_err(got, want)
    print(name, "rel err", err, "bound", ATTN_BOUND)
    assert err < ATTN_BOUND, (name, err)


def test_attention_masked_launcher_directly():
    """vx_attention_masked_f16 on head-major operands: q pre-scaled by scale * log2(e), an f32 per-head mask shared by the batch (Bm = 1), T = 64
    (aligned mask rows: the 16-byte loads), with a band that masks the whole first key block of the late queries."""
    hd, H, T, B = 64, 2, 64, 2
    rng = np.random.default_rng(9)
    q, k, v = (R.f16(rng.standard_normal((B, H, T, hd)) * 0.8) for _ in range(3))
    mask = (rng.standard_normal((1, H, T, T)) * 1.0).astype(np.float32).astype(np.float64) + _band(T, 9)[None, None]
    qs = R.f16(q * (math.log2(math.e) / math.sqrt(hd)))
    out = empty(B * T * H * hd * 2)
    args = [dev(a.astype(np.float16)).ptr for a in (qs, k, v)] + [dev(mask.astype(np.float32)).ptr, out.ptr]
    L.vx_check(api().vx_attention_masked_f16(*args, B, H, T, hd, H, 1, 1, None))
    sync()
    got = out.to_numpy(np.float16, (B, T, H * hd)).astype(np.float64)
    want = R.attention_masked(qs.transpose(0, 2, 1, 3), k.transpose(0, 2, 1, 3), v.transpose(0, 2, 1, 3), mask, math.log(2.0))
    assert R.rel_err(got, want) < ATTN_BOUND
    for bad, msg in [((B, H, T, 48, H, 1), b"head_dim 48"), ((B, H, T, hd, 3, 1), b"mask has 3 heads"), ((3, H, T, hd, H, 2), b"does not divide")]:
        assert api().vx_attention_masked_f16(*args, *bad, 1, None) == 0 and msg in api().vx_last_error(), msg


# ---- split_qkv ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("split_dim", [1, 2])
def test_split_qkv_against_numpy(device, split_dim):
    """nn.cpp:182-208 on a 96 -> 288 linear, 3 heads, T = 10, B = 2. The product is one f16 rounding (2^-11) of an f32 sum away from float64:
    bound 2 * 2^-11 = 1e-3 relative to the largest value; the split itself is data movement of that product."""
    C, heads, T, B = 96, 3, 10, 2
    hd = C // heads
    rng = np.random.default_rng(split_dim)
    x = R.f16(rng.standard_normal((B, T, C)))
    w, b = R.f16(rng.standard_normal((3 * C, C)) * 0.1), (rng.standard_normal(3 * C) * 0.1).astype(np.float32)
    g = G.Graph(device)
    g.add_weight("qkv.weight", w, G.F16)
    g.add_weight("qkv.bias", b, G.F32)
    xi = g.input((C, T, B), G.F16)
    parts = G.split_qkv(G.ModelRef(g, "qkv"), xi, heads, split_dim)
    assert all(p.ne == (hd, heads, T, B) for p in parts)
    for p, n in zip(parts, "qkv"):
        g.output(p, n)
    g.allocate()
    g.set(xi, x)
    g.compute()
    y = x @ w.T + b.astype(np.float64)  # [B, T, 288]
    y = y.reshape(B, T, heads, 3, hd).transpose(3, 0, 1, 2, 4) if split_dim == 1 else y.reshape(B, T, 3, heads, hd).transpose(2, 0, 1, 3, 4)
    for i, p in enumerate(parts):
        assert R.rel_err(g.get(p), y[i]) < 1e-3, (split_dim, i)


# ---- the SWIN encoder through the graph layer -------------------------------------------------------------------------------------------

MEAN = np.array([0.485, 0.456, 0.406], np.float32)
STD = np.array([0.229, 0.224, 0.225], np.float32)
ENC_W, ENC_H = 256, 288  # maps 64x72, 32x36, 16x18, 8x9: every stage pads its windows and carries shift masks


def test_swin_encode_every_block_against_the_oracle(device, tmp_path):
    cfg = synth.SWIN_MINI
    path = synth.write_swin_gguf(tmp_path / "mini.gguf", cfg, seed=5)
    tensors, conv_idx = synth.swin_gguf_tensors(synth.swin_state_dict(cfg, 5))
    om, P = oracle.Model(tensors, conv_idx), oracle.swin_params(cfg.embed_dim, cfg.window_size, cfg.depths, cfg.n_heads)
    imgs = synth.images(2, ENC_W, ENC_H, seed=11)
    pre = ((imgs.astype(np.float32) / 255.0 - MEAN) / STD).astype(np.float32)  # birefnet_process_input (birefnet.cpp:259-270)

    g = G.Graph(device, G.Weights(path))
    m = G.ModelRef(g, "bb")
    image = g.input((3, ENC_W, ENC_H, 2), G.F32, "image")
    G.swin_precompute(m, (ENC_W, ENC_H), cfg.window_size)
    outs = G.swin_encode(m, image, cfg.window_size, cfg.depths, cfg.n_heads)
    for i, o in enumerate(outs):
        g.output(o, f"out{i}")
    blocks = {f"block_{l}_{b}": g.output(g.get_tensor(f"bb.layers.{l}.blocks.{b}"), f"block_{l}_{b}") for l in range(4) for b in range(cfg.depths[l])}
    g.use_hip_graph(True)
    g.allocate()
    lines = g.describe().splitlines()
    assert sum(l.startswith("attention_masked") for l in lines) == sum(cfg.depths)
    g.set(image, pre)
    g.compute()
    got_outs = [g.get(o) for o in outs]
    got_blocks = {n: g.get(t).reshape(2, -1) for n, t in blocks.items()}  # [C, tokens, B] -> per image, row = y * w + x
    sizes = {n: (64 >> int(n[6])) * (72 >> int(n[6])) * (32 << int(n[6])) for n in blocks}
    for bi in range(2):
        want, caps = oracle.swin_encode(om, P, pre[bi], "bb", captures=sizes)
        for n in blocks:
            err = R.rel_err(got_blocks[n][bi], caps[n])
            assert err < 6e-3, (bi, n, err)
        for i in range(4):
            assert got_outs[i].shape[1:] == want[i].shape
            assert R.rel_err(got_outs[i][bi], want[i]) < 1e-2, (bi, i)
            assert np.abs(got_outs[i][bi] - want[i]).mean() < 2e-3 * np.abs(want[i]).max(), (bi, i)
    # the second compute replays the launch list as one hipGraph: bit-identical
    g.compute()
    for i, o in enumerate(outs):
        np.testing.assert_array_equal(g.get(o), got_outs[i])
    for n, t in blocks.items():
        np.testing.assert_array_equal(g.get(t).reshape(2, -1), got_blocks[n])

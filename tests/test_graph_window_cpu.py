"""The graph layer's window ops without a GPU (`Graph(None)`): shape inference of PERMUTE / ROLL / PAD / GET_ROWS / CAST /
ATTENTION_MASKED against numpy, host folding of the constant chain swin::window_attention builds (swin.cpp:72-90), the refusals, the
planned launch list of one shifted SWIN block, and the C++ face (tests/cpp/window_check.cpp) against the Python face."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import graph_cases as GC
import graph_window_ref as R
from oracle import oracle
from visioncpp_amd import _lib as L
from visioncpp_amd import graph as G
from visioncpp_amd import synth


def _g():
    return G.Graph(None)


def test_shape_inference_of_the_window_ops_follows_numpy():
    g = _g()
    m = G.ModelRef(g)
    ne = (24, 5, 7, 2)
    x = g.input(ne, G.F16)
    a = np.zeros(ne[::-1])
    for axes in [(0, 2, 1, 3), (1, 0, 2, 3), (2, 0, 1, 3), (3, 2, 1, 0), (1, 2, 3, 0)]:  # all but the first move ne[0]
        assert G.permute(m, x, *axes).ne == R.permute(a, axes).shape[::-1], axes
    assert G.permute(m, x, 2, 0, 1, 3).ne == (5, 7, 24, 2)  # ggml: source dimension 0 becomes dimension 2
    for shifts in [(0, -3, -3, 0), (5, 0, 9, -1), (-25, 7, 0, 3)]:
        assert G.roll(m, x, *shifts).ne == ne
    assert G.pad(m, x, 0, 2, 0, 0).ne == R.pad(a, (0, 2, 0, 0)).shape[::-1] == (24, 7, 7, 2)
    assert G.pad(m, x, 3, 0, 1, 2).ne == (27, 5, 8, 4)
    assert G.cast(m, x, G.F16).ne == ne and G.cast(m, x, G.F16).dtype == G.F16
    table = g.add_weight("table", np.zeros((169, 3), np.float32))
    idx = g.add_weight("idx", np.zeros((49, 49), np.int32), G.I32)
    rows = G.get_rows(m, table, idx)
    assert rows.ne == (3, 49, 49, 1) and rows.dtype == G.F32 and rows.is_constant  # ggml: get_rows gives f32
    q = g.input((32, 3, 49, 8), G.F16)
    for mask_ne in [(49, 49, 3, 4), (49, 49, 1, 1), (49, 49, 1, 8)]:
        assert g.op(G.OP_ATTENTION_MASKED, [q, q, q, g.input(mask_ne, G.F16)], fparams=[0.1]).ne == (96, 49, 8, 1)
    for bad, msg in [(lambda: G.permute(m, x, 0, 1, 1, 3), "permute: the axes"), (lambda: G.pad(m, x, 0, -1, 0, 0), "pad: four non-negative"),
                     (lambda: G.cast(m, x, G.F32), "cast: an f16 activation to f32"), (lambda: G.cast(m, x, 7), "cast: the target type"),
                     (lambda: G.get_rows(m, table, g.add_weight("fidx", np.zeros(4, np.float32))), "get_rows: the index is an i32 constant")]:
        with pytest.raises(L.Error, match=msg):
            bad()


def test_fold_helpers_match_numpy_on_constants():
    """permute / roll / pad on constants are evaluated on the host: values, not only shapes (negative and wrapping shifts included)."""
    g = _g()
    m = G.ModelRef(g)
    rng = np.random.default_rng(0)
    a = rng.standard_normal((2, 3, 5, 6)).astype(np.float32)
    c = g.add_weight("c", a, G.F32)
    for axes in [(0, 2, 1, 3), (2, 0, 1, 3), (3, 2, 1, 0), (1, 2, 3, 0)]:
        np.testing.assert_array_equal(g.read_constant(G.permute(m, c, *axes)), R.permute(a, axes))
    for shifts in [(0, -3, -3, 0), (5, 0, 9, -1), (-13, 2, 0, 1)]:
        np.testing.assert_array_equal(g.read_constant(G.roll(m, c, *shifts)), R.roll(a, shifts))
    np.testing.assert_array_equal(g.read_constant(G.pad(m, c, 2, 0, 1, 3)), R.pad(a, (2, 0, 1, 3)))
    half = g.read_constant(G.cast(m, c, G.F16))
    np.testing.assert_array_equal(half, a.astype(np.float16).astype(np.float32))


def test_window_attention_constants_fold_into_one_mask():
    """get_rows -> reshape -> permute -> cast -> add(repeat(mask)) on constants (swin.cpp:72-90) is ONE constant: table[index] + mask, for
    ws = 7, 3 heads and the mask of a 2 x 2-window map, two images."""
    ws, heads, n = 7, 3, 49
    g = _g()
    m = G.ModelRef(g)
    rng = np.random.default_rng(1)
    table = (rng.standard_normal(((2 * ws - 1) ** 2, heads)) * 0.5).astype(np.float32)
    g.add_weight("attn.relative_position_bias_table", table, G.F32)
    index, mask = G.swin_relative_position_index(ws), G.swin_attention_mask(14, 14, ws)
    np.testing.assert_array_equal(index, oracle.swin_rel_pos_index(ws))
    np.testing.assert_array_equal(mask, oracle.swin_attention_mask(14, 14, ws))
    for w, h in [(64, 72), (8, 9), (5, 20)]:
        np.testing.assert_array_equal(G.swin_attention_mask(w, h, ws), oracle.swin_attention_mask(w, h, ws))
    G.swin_precompute(m, (56, 56), ws, 0)
    assert g.get_tensor("window_attention_7.rel_pos_index").dtype == G.I32
    mt = g.get_tensor("swin_layer_14x14.attn_mask")
    assert mt is not None and mt.ne == (n, n, 4, 1)
    b = 8  # 4 windows x 2 images
    bias = G.cast(m, G.permute(m, G.reshape(m, G.get_rows(m, g.find("attn.relative_position_bias_table"), g.get_tensor("window_attention_7.rel_pos_index")),
                                            heads, n, n, 1), 2, 0, 1, 3), G.F16)
    mk = G.repeat(m, G.reshape(m, mt, n, n, 4, 1), n, n, 4, 2)
    mk = G.repeat(m, G.reshape(m, mk, n, n, 1, b), n, n, heads, b)
    total = G.add(m, mk, bias)
    assert total.is_constant and total.ne == (n, n, heads, b)
    want_bias = table.astype(np.float16).astype(np.float32)[index.reshape(n, n)].transpose(2, 0, 1)  # [heads, query, key]
    np.testing.assert_array_equal(g.read_constant(bias)[0], want_bias)
    want = want_bias[None] + mask[np.arange(b) % 4][:, None]
    got = g.read_constant(total)
    np.testing.assert_array_equal(got, want)
    assert np.isneginf(got).any() and not np.isnan(got).any()


def _qkv(g, hd, heads, T, B):
    return [g.input((hd, heads, T, B), G.F16, f"{n}{hd}_{heads}_{T}_{B}") for n in "qkv"]


def test_refusals_name_the_op():
    g = _g()
    q, k, v = _qkv(g, 32, 3, 49, 8)
    with pytest.raises(L.Error, match="attention_masked: the mask has 2 heads"):
        g.op(G.OP_ATTENTION_MASKED, [q, k, v, g.input((49, 49, 2, 4), G.F16)], fparams=[1.0])
    with pytest.raises(L.Error, match="attention_masked: the mask's batch 3 does not divide the batch 8"):
        g.op(G.OP_ATTENTION_MASKED, [q, k, v, g.input((49, 49, 3, 3), G.F16)], fparams=[1.0])
    q48 = _qkv(g, 48, 2, 49, 2)
    with pytest.raises(L.Error, match="attention_masked: head_dim 48"):
        g.op(G.OP_ATTENTION_MASKED, q48 + [g.input((49, 49, 1, 1), G.F16)], fparams=[1.0])
    k50 = g.input((32, 3, 50, 8), G.F16, "k50")
    with pytest.raises(L.Error, match=r"attention_masked: 49 queries on 50 keys; cross-attention \(T_q != T_k\) is not built"):
        g.op(G.OP_ATTENTION_MASKED, [q, k50, k50, g.input((50, 49, 1, 1), G.F16)], fparams=[1.0])
    # the 3-source op keeps its refusal of everything but head_dim 64 (at allocate time)
    g2 = _g()
    q2 = _qkv(g2, 32, 3, 49, 8)
    g2.output(g2.op(G.OP_ATTENTION, q2, fparams=[1.0]))
    with pytest.raises(L.Error, match="the fused kernel is built for head_dim 64 self-attention"):
        g2.allocate()
    # get_rows on an activation: built, refused when the graph is lowered
    g3 = _g()
    m3 = G.ModelRef(g3)
    idx = g3.add_weight("idx", np.arange(4, dtype=np.int32), G.I32)
    g3.output(G.get_rows(m3, g3.input((8, 16, 1, 1), G.F16, "table"), idx))
    with pytest.raises(L.Error, match="get_rows on activations is not built"):
        g3.allocate()
    g4 = _g()
    table = g4.add_weight("t", np.zeros((4, 8), np.float32))
    with pytest.raises(L.Error, match="get_rows: index 4 at position 1 is outside the table's 4 rows"):
        G.get_rows(G.ModelRef(g4), table, g4.add_weight("idx", np.array([0, 4], np.int32), G.I32))


def _block_graph(tmp_path):
    """bb.layers.0.blocks.1 of SWIN_MINI (C = 32, one head, shift 3) on a 14 x 14 map, two images."""
    path = synth.write_swin_gguf(tmp_path / "mini.gguf", synth.SWIN_MINI, seed=5)
    g = G.Graph(None, G.Weights(path))
    GC.swin_block_mini(g)
    g.allocate()
    return path, g


def test_planned_swin_block_has_one_attention_launch_and_no_mask_chain(tmp_path):
    _, g = _block_graph(tmp_path)
    lines = g.describe().strip().splitlines()[:-1]
    att = [l for l in lines if l.startswith("attention")]
    assert att == ["attention_masked B=8 heads=1 T=49 hd=32 mask=[1, 4] (constant)"], att  # folded for 8 windows, uploaded once per image's 4
    # the constant chain (get_rows, reshape, permute, cast, repeat, add) never reaches the device
    assert not [l for l in lines if l.startswith(("get_rows", "cast", "repeat"))], lines
    assert [l for l in lines if l.startswith("add ")] == ["add n=12544 period=12544"]  # the block's shortcut, [32, 196, 2]; not the mask + bias sum
    assert sum(l.startswith("permute") for l in lines) == 3  # window partition, q|k|v split, window reverse
    assert sum(l.startswith("roll") for l in lines) == 2 and not any(l.startswith("pad ") for l in lines)  # 14 = 2 x 7: no padding
    assert [l for l in lines if l.startswith("roll")][0] == "roll [32, 14, 14, 2] by [0, -3, -3, 0]"
    assert sum(l.startswith("gemm") for l in lines) == 4  # qkv, proj, fc1[gelu], fc2[+res]


def test_cpp_face_builds_the_same_block(tmp_path):
    """tests/cpp/window_check.cpp: the block through include/visp/nn.h with VISP_GGML_NAMES, planned on the host; its launch list equals the Python face's."""
    path, g = _block_graph(tmp_path)
    exe = Path(__file__).resolve().parents[1] / "vision.cpp_amd" / "lib" / "window_check"
    assert exe.exists(), "built by __graft_entry__.build()"
    r = subprocess.run([str(exe), str(path), "bb.layers.0.blocks.1", "32", "1", "14", "14", "2", "7"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout, r.stderr)
    assert r.stdout == g.describe()


def test_swin_encode_plans_with_padding_and_masks_at_every_stage(tmp_path):
    """swin_encode of SWIN_MINI at 256 x 288 (maps 64x72 .. 8x9: every stage pads): one masked attention per block, all masks constants."""
    cfg = synth.SWIN_MINI
    path = synth.write_swin_gguf(tmp_path / "mini.gguf", cfg, seed=5)
    g = G.Graph(None, G.Weights(path))
    outs = GC.swin_encode_mini(g)["outs"]
    assert [o.ne for o in outs] == [(32, 64, 72, 2), (64, 32, 36, 2), (128, 16, 18, 2), (256, 8, 9, 2)]
    g.allocate()
    lines = g.describe().strip().splitlines()[:-1]
    att = [l for l in lines if l.startswith("attention")]
    assert len(att) == sum(cfg.depths) and all("(constant)" in l and "hd=32" in l for l in att)
    assert sum(l.startswith("pad ") for l in lines) == sum(cfg.depths) and sum(l.startswith("roll") for l in lines) == sum(cfg.depths)

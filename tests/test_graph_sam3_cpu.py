"""The graph layer's ROPE op, get_rows with a run-time index, repeat that tiles constants and the SAM3 / CLIP builders without a GPU (`Graph(None)`): shape
inference, host folding, every refusal by its message, the planned launch lists of one window layer, one global layer, the mini vision encoder and the mini
text encoder with fused models and per node, recorded as they come out, and the C++ face (tests/cpp/sam3_check.cpp) against the Python face."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

from visioncpp_amd import _lib as L
from visioncpp_amd import graph as G
from visioncpp_amd import synth

ROOT = Path(__file__).resolve().parents[1]
VIT, CLIP = synth.SAM3_VIT_MINI, synth.CLIP_TEXT_MINI


@pytest.fixture(scope="module")
def gguf(tmp_path_factory):
    return synth.write_sam3_gguf(tmp_path_factory.mktemp("sam3") / "sam3_mini.gguf", VIT, CLIP, seed=1)


def _lines(g):
    return g.describe().strip().splitlines()[:-1]


def _kinds(g):
    return [l.split(" ")[0] for l in _lines(g)]


def _new(path, fused):
    g = G.Graph(None, G.Weights(path))
    g.set_fused_models(fused)
    return g, G.ModelRef(g)


def _pos(g, T, name="pos"):
    return g.add_weight(name, np.arange(T, dtype=np.int32), G.I32)


# ---- the op ------------------------------------------------------------------------------------------------------------------------------------------------

def test_op_value_and_shapes():
    assert G.OP_ROPE == 42
    g = G.Graph(None)
    m = G.ModelRef(g)
    for ne in [(32, 2, 16, 3), (64, 1, 1, 1), (8, 3, 25, 2)]:
        x = g.input(ne, G.F16, f"x{ne}")
        y = G.rope(m, x, _pos(g, ne[2], f"p{ne}"), ne[0], 10000.0, 0.5)
        assert y.ne == ne and y.dtype == G.F16 and not y.is_constant
    q = g.input((64, 2, 16, 3), G.F16, "q")
    pos = G.sam3_rope_2d_positions(m, 16, 4, 1.0, "_vit_rope_pos_window")
    assert g.get_tensor("_vit_rope_pos_window.x").index == pos.x.index and pos.x.dtype == G.I32 and pos.x.is_constant and pos.y.ne == (16, 1, 1, 1)
    assert G.sam3_apply_rope_2d(m, q, pos).ne == (64, 2, 16, 3)
    assert G.sam3_rope_2d_positions(m, 16, 4, 1.0, "_vit_rope_pos_window").x.index == pos.x.index  # made once per name


def test_rope_refusals():
    g = G.Graph(None)
    m = G.ModelRef(g)
    x = g.input((32, 2, 16, 3), G.F16, "x")
    pos = _pos(g, 16)
    bad = [
        (lambda: G.rope(m, x, pos, 16, 1e4, 1.0), "rope: n_dims 16 on rows of 32 channels"),
        (lambda: G.rope(m, g.input((12, 2, 16, 3), G.F16, "x12"), pos, 12, 1e4, 1.0), "rope: rows of 12 channels"),
        (lambda: G.rope(m, x, g.input((16,), G.I32, "ipos"), 32, 1e4, 1.0), "rope: the positions are an i32 constant"),
        (lambda: G.gelu(m, g.input((16,), G.I32, "ival")), "gelu: operand 0 is an i32 graph input; an i32 tensor is an index, not a value"),
        (lambda: G.add(m, x, g.input((32, 2, 16, 3), G.I32, "iadd")), "add: operand 1 is an i32 graph input"),
        (lambda: G.rope(m, x, g.add_weight("fpos", np.zeros(16, np.float32), G.F32), 32, 1e4, 1.0), "rope: the positions are an i32 constant"),
        (lambda: G.rope(m, x, _pos(g, 15, "p15"), 32, 1e4, 1.0), "rope: positions .* do not match the 16 tokens"),
        (lambda: G.rope(m, g.add_weight("cx", np.zeros((3, 16, 2, 32), np.float32)), pos, 32, 1e4, 1.0), "rope: x is a constant"),
        (lambda: G.rope(m, g.input((32, 2, 16, 3), G.F32, "xf"), pos, 32, 1e4, 1.0), "rope: x is f32"),
        (lambda: g.op(G.OP_ROPE, [x, pos], [32, 2], [1e4, 1.0]), "rope: mode 2 is not built"),
        (lambda: g.op(G.OP_ROPE, [x, pos], [32, 0], [1e4]), "rope: one or two integer parameters"),
        (lambda: g.op(G.OP_ROPE, [x], [32, 0], [1e4, 1.0]), "rope: takes 2..2 tensors"),
        (lambda: G.rope(m, x, pos, 32, 0.0, 1.0), "rope: freq_base 0"),
    ]
    for fn, msg in bad:
        with pytest.raises(L.Error, match=msg):
            fn()


# ---- get_rows and repeat ---------------------------------------------------------------------------------------------------------------------------------------

def test_get_rows_with_a_runtime_index():
    g = G.Graph(None)
    m = G.ModelRef(g)
    table = np.random.default_rng(0).standard_normal((10, 16)).astype(np.float32)
    t = g.add_weight("table", table)
    for ne, want in [((8,), (16, 8, 1, 1)), ((8, 3), (16, 8, 3, 1))]:
        y = G.get_rows(m, t, g.input(ne, G.I32, f"ids{len(ne)}"))
        assert y.ne == want and y.dtype == G.F16 and not y.is_constant
    # everything refused before stays refused with its text; a constant index still folds to f32, bit for bit
    with pytest.raises(L.Error, match=r"get_rows: the index is an i32 constant \(visp_graph_add_weight with dtype 26\)"):
        G.get_rows(m, t, g.add_weight("fidx", np.zeros(4, np.float32)))
    with pytest.raises(L.Error, match="get_rows: the index is an i32 constant"):
        G.get_rows(m, t, g.input((4,), G.F16, "hidx"))
    with pytest.raises(L.Error, match="get_rows: a table of 12 channels with a run-time index"):
        G.get_rows(m, g.add_weight("t12", np.zeros((4, 12), np.float32)), g.input((4,), G.I32, "i12"))
    idx = np.array([[0, 9], [3, 3]], np.int32)
    c = G.get_rows(m, t, g.add_weight("cidx", idx, G.I32))
    assert c.is_constant and c.dtype == G.F32 and c.ne == (16, 2, 2, 1)
    assert np.array_equal(g.read_constant(c)[0].view(np.uint32), table[idx].view(np.uint32))
    # a non-constant table: refused when the graph is lowered, with the text it had
    g2 = G.Graph(None)
    g2.output(G.get_rows(G.ModelRef(g2), g2.input((8, 16), G.F16, "table"), g2.input((4,), G.I32, "ids")))
    with pytest.raises(L.Error, match="get_rows on activations is not built"):
        g2.allocate()
    g3 = G.Graph(None)
    g3.output(G.get_rows(G.ModelRef(g3), g3.add_weight("t", table), g3.input((8, 2), G.I32, "ids")), "rows")
    g3.allocate()
    assert _lines(g3) == ["get_rows rows=10 C=16 n=16 <- t"]


def test_repeat_tiles_constants_only():
    g = G.Graph(None)
    m = G.ModelRef(g)
    a = np.random.default_rng(1).standard_normal((1, 4, 4, 8)).astype(np.float32)
    t = G.repeat(m, g.add_weight("pos", a, G.F32), 8, 8, 12, 2)
    assert t.is_constant and t.ne == (8, 8, 12, 2)
    assert np.array_equal(g.read_constant(t), np.tile(a, (2, 3, 2, 1)))
    with pytest.raises(L.Error, match="repeat: .* to .* \\(source dimensions must be 1 or already equal\\)"):
        G.repeat(m, g.add_weight("pos3", a[:, :3], G.F32), 8, 8, 8, 1)  # 8 is no multiple of 3
    with pytest.raises(L.Error, match=r"repeat: \[8, 4, 4, 1\] to \[8, 8, 8, 1\] \(source dimensions must be 1 or already equal\)"):
        G.repeat(m, g.input((8, 4, 4, 1), G.F16, "act"), 8, 8, 8, 1)


def test_vision_embed_tiles_the_position_embedding(gguf):
    g, m = _new(gguf, True)
    e = G.sam3_vision_embed(m["det.ve.backbone.embeddings"], g.input((3, 16, 16, 2), G.F32, "image"), VIT.patch)
    assert e.ne == (VIT.hidden, 64, 2, 1)
    g.output(e, "embed")
    g.allocate()
    assert _kinds(g) == ["im2col_patches", "gemm", "add"]  # the tiled position embedding never reaches the device as a repeat


# ---- launch lists ----------------------------------------------------------------------------------------------------------------------------------------------

def _layer(path, fused, window, grid=8, batch=1, layer=0):
    g, m = _new(path, fused)
    x = g.input((VIT.hidden, grid, grid, batch), G.F16, "x")
    n = window if window else grid
    pos = G.sam3_rope_2d_positions(m, n * n, n, 1.0 if window else 0.5, "_vit_rope_pos_window" if window else "_vit_rope_pos_global")
    g.output(G.sam3_vision_layer(m["det.ve.backbone.layers"][layer], x, window, VIT.heads, pos), "y")
    g.allocate()
    return g


ATTN_FUSED = ["gemm[qkv", "rope_2d[q", "attention"]
ATTN_PER_NODE = ["gemm", "gemm", "gemm"] + ["slice", "rope", "slice", "rope", "concat", "concat"] * 2 + ["heads_major"] * 3 + ["attention"]
TAIL = ["gemm", "add", "layer_norm", "gemm[gelu]", "gemm[+res]"]


def test_layer_launch_lists(gguf):
    assert _kinds(_layer(gguf, True, 4)) == ["layer_norm", "permute"] + ATTN_FUSED + ["gemm", "permute"] + TAIL[1:]
    assert _kinds(_layer(gguf, True, 0)) == ["layer_norm"] + ATTN_FUSED + TAIL
    assert _kinds(_layer(gguf, False, 4)) == ["layer_norm", "permute"] + ATTN_PER_NODE + ["gemm", "permute"] + TAIL[1:]
    assert _kinds(_layer(gguf, False, 0)) == ["layer_norm"] + ATTN_PER_NODE + TAIL
    assert _kinds(_layer(gguf, True, 4, grid=6)) == ["layer_norm", "pad", "permute"] + ATTN_FUSED + ["gemm", "permute", "slice"] + TAIL[1:]
    fused = _lines(_layer(gguf, True, 4, batch=2))
    assert fused[2:5] == ["gemm[qkv heads-major] M=128 N=384 K=128 <- det.ve.backbone.layers.0.attention.q_proj.weight",
                          "rope_2d[q k heads-major, in place] hd=64 heads=2 T=16 B=8", "attention B=8 heads=2 T=16"]
    per_node = _lines(_layer(gguf, False, 4, batch=2))
    assert per_node.count("rope n=32 heads=2 T=16 B=8") == 4 and not [l for l in per_node if l.startswith("rope_2d")]
    assert not [l for l in fused if l.startswith(("heads_major", "slice", "concat", "rope "))]


def test_rope_2d_group_on_its_own_is_one_launch():
    """The group without the q|k|v chain around it (q comes from a graph input): one launch with fused models, six per node."""
    for fused, want in [(True, ["rope_2d"]), (False, ["slice", "rope", "slice", "rope", "concat", "concat"])]:
        g = G.Graph(None)
        g.set_fused_models(fused)
        m = G.ModelRef(g)
        pos = G.sam3_rope_2d_positions(m, 25, 5, 1.0, "p")
        g.output(G.sam3_apply_rope_2d(m, g.input((64, 3, 25, 2), G.F16, "q"), pos), "out")
        g.allocate()
        assert _kinds(g) == want
    # ropes with different scales are not the group
    g = G.Graph(None)
    m = G.ModelRef(g)
    q = g.input((64, 3, 25, 2), G.F16, "q")
    pos = G.sam3_rope_2d_positions(m, 25, 5, 1.0, "p")
    g.output(G.concat(m, [G.rope(m, G.slice_(m, q, (0, 32)), pos.x, 32, 1e4, 1.0), G.rope(m, G.slice_(m, q, (32, 64)), pos.y, 32, 1e4, 0.5)], 0), "out")
    g.allocate()
    assert _kinds(g) == ["slice", "rope", "slice", "rope", "concat", "concat"]


def _vision(path, fused, batch=2):
    g, m = _new(path, fused)
    image = g.input((3, VIT.image_size, VIT.image_size, batch), G.F32, "image")
    p = G.Sam3VitParams(VIT.image_size, VIT.patch, VIT.window, VIT.n_layers, VIT.heads, VIT.global_layers)
    hidden, pos = G.sam3_encode_vision(m["det.ve"], image, p)
    for i, h in enumerate(hidden):
        g.output(h, f"fpn_{i}")
    g.allocate()
    return g, hidden, pos


def test_vision_encoder_launch_lists(gguf):
    g, hidden, pos = _vision(gguf, True)
    assert [h.ne for h in hidden] == [(32, 32, 32, 2), (32, 16, 16, 2), (32, 8, 8, 2), (32, 4, 4, 2)]
    assert [p.ne for p in pos] == [(32, 32, 32, 1), (32, 16, 16, 1), (32, 8, 8, 1), (32, 4, 4, 1)] and all(p.is_constant and p.dtype == G.F32 for p in pos)
    kinds = _kinds(g)
    assert kinds[:4] == ["im2col_patches", "gemm", "add", "layer_norm"]
    assert kinds[4:15] == ["layer_norm", "permute"] + ATTN_FUSED + ["gemm", "permute"] + TAIL[1:]
    assert kinds[15:24] == ["layer_norm"] + ATTN_FUSED + TAIL
    assert len(kinds) == 38 and kinds.count("rope_2d[q") == 2
    per_node = _kinds(_vision(gguf, False)[0])
    assert len(per_node) == 70 and per_node.count("rope") == 8 and per_node.count("heads_major") == 6


def _text(path, fused, batch=2):
    g, m = _new(path, fused)
    ids, mask = g.input((CLIP.positions, batch), G.I32, "ids"), g.input((CLIP.positions, CLIP.positions, 1, 1), G.F16, "mask")
    g.output(G.sam3_encode_text(m["det"], ids, mask, CLIP.heads), "text")
    g.allocate()
    return g


def test_text_encoder_launch_lists(gguf):
    layer = ["layer_norm", "gemm", "gemm", "gemm", "heads_major", "heads_major", "heads_major", "attention_masked", "gemm[+res]", "layer_norm", "gemm[gelu]", "gemm[+res]"]
    for fused in (True, False):
        g = _text(gguf, fused)
        assert _kinds(g) == ["get_rows", "add"] + layer * CLIP.n_layers + ["layer_norm", "gemm"]
        assert _lines(g)[0] == "get_rows rows=100 C=128 n=16 <- det.te.text_model.embeddings.token_embedding.weight"
        assert _lines(g)[9] == "attention_masked B=2 heads=2 T=8 hd=64 mask=[1, 1] f16"


def test_existing_attention_chains_match_as_before():
    """A graph without a ROPE node: the q|k|v chain of three linears over one input is found as it was."""
    g = G.Graph(None)
    m = G.ModelRef(g)
    rng = np.random.default_rng(2)
    for n in ("q", "k", "v", "o"):
        g.add_weight(f"{n}.weight", rng.standard_normal((128, 128)).astype(np.float32))
    x = g.input((128, 16, 2), G.F16, "x")
    q, k, v = (G.reshape(m, G.linear(m[n], x), 64, 2, 16, 2) for n in ("q", "k", "v"))
    g.output(G.attention(m, q, k, v, None, 0.125, m["o"]), "y")
    g.allocate()
    assert _kinds(g) == ["gemm[qkv", "attention", "gemm"]


# ---- the C++ face ----------------------------------------------------------------------------------------------------------------------------------------------

def test_cpp_face_builds_the_same_layer(gguf):
    """tests/cpp/sam3_check.cpp: one vision layer through include/visp/nn.h with ggml_rope_ext under VISP_GGML_NAMES; describe() line by line against the Python face."""
    exe = ROOT / "vision.cpp_amd" / "lib" / "sam3_check"
    assert exe.exists(), "built by __graft_entry__.build()"
    for fused in (True, False):
        for layer, grid, window, batch in [(0, 8, 4, 1), (1, 8, 0, 2), (0, 6, 4, 2)]:
            r = subprocess.run([str(exe), str(gguf), str(layer), str(VIT.heads), str(grid), str(window), str(batch), str(int(fused))], capture_output=True, text=True, timeout=120)
            assert r.returncode == 0, r.stderr
            want = _layer(gguf, fused, window, grid, batch, layer)
            assert r.stdout.strip().splitlines()[:-1] == _lines(want)
    # the ggml-named wrapper refuses what is not built, by the op's name
    for code, msg in [(-1, "rope: ext_factor"), (-2, "rope: ext_factor"), (-3, "rope: ext_factor"), (-4, "rope: ext_factor"), (-5, "rope: frequency factors"), (-6, "rope: mode 2 is not built")]:
        r = subprocess.run([str(exe), str(gguf), str(code), "2", "4", "4", "1", "1"], capture_output=True, text=True, timeout=120)
        assert r.returncode == 1 and msg in r.stderr, (code, r.stderr)
    r = subprocess.run([str(exe), str(gguf), "0", "4", "8", "4", "1", "1"], capture_output=True, text=True, timeout=120)  # head_dim 32: halves of 16 channels rotate, the attention refuses
    assert r.returncode == 1 and "head_dim" in r.stderr

"""The graph layer's depthwise conv and the TinyViT builders without a GPU (`Graph(None)`): shape inference against numpy in both stored kernel
forms, every refusal by its message, the planned launch lists of a depthwise + gelu pair, of a tinyvit_block (fused: one window_attention on the q|k|v
product's rows; per node: one attention_masked), of a SWIN block (unchanged by this layer's new match), of patch_embed on the f32 image, the whole
mini encoder, and the C++ face (tests/cpp/tinyvit_check.cpp) against the Python face."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import dwconv_ref as R
from visioncpp_amd import _lib as L
from visioncpp_amd import graph as G
from visioncpp_amd import synth

KSP = [(3, 1, 1), (3, 2, 1), (4, 1, 2), (4, 2, 1), (5, 1, 2), (7, 1, 3), (1, 1, 0)]


def _dw(g, name, w, form, bias=None):
    """kernel w [k, k, C] as a weight `name`.weight in stored form 0 ([C, 1, kw, kh]) or 1 ([1, kw, kh, C]) -> its ModelRef"""
    g.add_weight(f"{name}.weight", np.asarray(R.kernel_forms(w)[form], np.float32))
    if bias is not None:
        g.add_weight(f"{name}.bias", np.asarray(bias, np.float32), G.F32)
    return G.ModelRef(g, name)


@pytest.mark.parametrize("form", [0, 1])
def test_shape_inference_follows_numpy(form):
    g = G.Graph(None)
    B, h, w, C = 2, 5, 7, 16
    x = g.input((C, w, h, B), G.F16, "x")
    for i, (k, stride, pad) in enumerate(KSP):
        want = R.depthwise_conv2d(np.zeros((B, h, w, C)), np.zeros((k, k, C)), None, stride, pad).shape
        t = G.conv_2d_depthwise(_dw(g, f"w{i}", np.zeros((k, k, C)), form, np.zeros(C) if i % 2 else None), x, stride, pad)
        assert t.ne == want[::-1] and t.dtype == G.F16 and not t.is_constant, (k, stride, pad)
    assert G.OP_CONV_2D_DEPTHWISE == 31
    assert G.conv_2d_depthwise(_dw(g, "even", np.zeros((4, 4, C)), form), x, 1, 2).ne == (C, w + 1, h + 1, B)


def test_refusals_name_the_op():
    g = G.Graph(None)
    m = G.ModelRef(g)
    C = 16
    x = g.input((C, 7, 5, 2), G.F16, "x")
    w3 = _dw(g, "w3", np.zeros((3, 3, C)), 0)
    with pytest.raises(L.Error, match="conv_2d_depthwise: stride 3 is not built"):
        G.conv_2d_depthwise(w3, x, 3, 1)
    g.add_weight("w32.weight", np.zeros((2, 3, 1, C), np.float32))  # ne [C, 1, kw = 3, kh = 2]
    with pytest.raises(L.Error, match="conv_2d_depthwise: kernel 3x2; square kernels only"):
        G.conv_2d_depthwise(G.ModelRef(g, "w32"), x, 1, 1)
    with pytest.raises(L.Error, match="conv_2d_depthwise: kernel 8x8; kernels up to 7x7"):
        G.conv_2d_depthwise(_dw(g, "w8", np.zeros((8, 8, C)), 1), g.input((C, 9, 9, 1), G.F16, "x9"), 1, 0)
    with pytest.raises(L.Error, match=r"conv_2d_depthwise: pad 3 with a 3x3 kernel \(0 \.\. k - 1\)"):
        G.conv_2d_depthwise(w3, x, 1, 3)
    x12 = g.input((12, 7, 5, 2), G.F16, "x12")
    with pytest.raises(L.Error, match="conv_2d_depthwise: C = 12 must be a multiple of 8"):
        G.conv_2d_depthwise(_dw(g, "w12", np.zeros((3, 3, 12)), 0), x12, 1, 1)
    with pytest.raises(L.Error, match="conv_2d_depthwise: the kernel must be a model weight"):
        m.graph.op(G.OP_CONV_2D_DEPTHWISE, [x, g.input((C, 1, 3, 3), G.F16, "w_act")], [1, 1])
    g.add_weight("dense.weight", np.zeros((C, 3, 3, C), np.float32))  # a dense conv kernel [Cin, kw, kh, Cout]
    with pytest.raises(L.Error, match=r"conv_2d_depthwise: kernel \[16, 3, 3, 16\] is neither \[C, 1, kw, kh\] nor \[1, kw, kh, C\]"):
        G.conv_2d_depthwise(G.ModelRef(g, "dense"), x, 1, 1)
    with pytest.raises(L.Error, match="conv_2d_depthwise: kernel .* is neither"):
        G.conv_2d_depthwise(_dw(g, "w24", np.zeros((3, 3, 24)), 1), x, 1, 1)  # another channel count
    with pytest.raises(L.Error, match="conv_2d_depthwise: bias has 8 elements, expected 16"):
        G.conv_2d_depthwise(_dw(g, "wb", np.zeros((3, 3, C)), 0, np.zeros(8)), x, 1, 1)
    with pytest.raises(L.Error, match="conv_2d_depthwise: a 7x7 kernel at pad 0 does not fit the 7x5 input"):
        G.conv_2d_depthwise(_dw(g, "w7", np.zeros((7, 7, C)), 0), x, 1, 0)
    # every other conv on a channel count that is no multiple of 8 is refused as before: only the 3-channel f32 image is new
    g.add_weight("c12.weight", np.zeros((8, 3, 3, 12), np.float32))
    g.output(G.conv_2d(G.ModelRef(g, "c12"), x12, 2, 1), "y")
    with pytest.raises(L.Error, match="Cin = 12 must be a multiple of 8"):
        g.allocate()
    with pytest.raises(L.Error, match="operand 0 is f32"):
        G.conv_2d_depthwise(_dw(g, "w8c", np.zeros((3, 3, 8)), 0), g.input((8, 7, 5, 2), G.F32, "xf32"), 1, 1)


def _pair(fused, act="gelu", form=0, k=3, stride=1, pad=1):
    g = G.Graph(None)
    m = _dw(g, "dw", np.zeros((k, k, 24)), form, np.zeros(24))
    x = g.input((24, 11, 7, 2), G.F16, "x")
    y = G.conv_2d_depthwise(m, x, stride, pad)
    g.output(G.gelu(m, y) if act == "gelu" else G.leaky_relu(m, y, 0.2), "y")
    g.set_fused_models(fused)
    g.allocate()
    return g.describe().strip().splitlines()[:-1]


def test_depthwise_and_its_activation_plan_as_one_launch_with_fused_models():
    assert _pair(True) == ["dwconv3x3[gelu] B=2 11x7 -> 11x7 C=24 pad=1 <- dw.weight"]
    assert _pair(False) == ["dwconv3x3 B=2 11x7 -> 11x7 C=24 pad=1 <- dw.weight", f"gelu n={2 * 7 * 11 * 24}"]
    assert _pair(True, "leaky", 1, 4, 2, 1) == ["dwconv4x4s2[leaky_relu] B=2 11x7 -> 5x3 C=24 pad=1 <- dw.weight"]
    assert _pair(False, "leaky", 1, 4, 2, 1) == ["dwconv4x4s2 B=2 11x7 -> 5x3 C=24 pad=1 <- dw.weight", f"leaky_relu n={2 * 3 * 5 * 24}"]
    # an activation with a second reader of the conv stays a launch
    g = G.Graph(None)
    m = _dw(g, "dw", np.zeros((3, 3, 8)), 0)
    y = G.conv_2d_depthwise(m, g.input((8, 6, 4, 1), G.F16, "x"), 1, 1)
    g.output(G.gelu(m, y), "a")
    g.output(G.scale(m, y, 2.0), "b")
    g.allocate()
    assert [l.split()[0] for l in g.describe().strip().splitlines()[:-1]] == ["dwconv3x3", "gelu", "scale"]


# ---- the TinyViT block and encoder of synth.TINYVIT_MINI ----------------------------------------------------------------------------------------

CFG = synth.TINYVIT_MINI
BLOCK = "enc.layers.2.blocks.1"  # C = 96, 3 heads, 14 x 14 windows on a 16 x 16 map (padded to 28): T = 196


@pytest.fixture(scope="module")
def gguf(tmp_path_factory):
    return synth.write_tinyvit_gguf(tmp_path_factory.mktemp("tinyvit") / "mini.gguf", CFG, seed=3)


def _block_graph(gguf, fused, batch=2):
    res, dim, _, heads, ws, _ = CFG.layers()[2]
    g = G.Graph(None, G.Weights(gguf))
    x = g.input((dim, res * res, batch), G.F16, "x")
    g.output(G.tinyvit_block(G.ModelRef(g, BLOCK), x, res, dim, heads, ws), "out")
    g.set_fused_models(fused)
    g.allocate()
    return g


def test_fused_block_runs_the_window_attention_on_the_qkv_rows(gguf):
    lines = _block_graph(gguf, True).describe().strip().splitlines()[:-1]
    assert [l for l in lines if l.startswith(("window_attention", "attention"))] == [f"window_attention windows=8 heads=3 T=196 hd=32 <- {BLOCK}.attn.qkv.weight"], lines
    assert not [l for l in lines if l.startswith(("heads_major", "slice [32"))]
    assert [l.split()[0] for l in lines] == ["pad", "permute", "layer_norm", "pad_rows", "gemm", "window_attention", "pad_rows", "gemm", "permute", "slice", "add", "dwconv3x3",
                                             "layer_norm", "pad_rows", "gemm[gelu]", "gemm[+res]"], lines
    assert lines[0] == "pad [96, 16, 16, 2] -> [96, 28, 28, 2]" and lines[9] == "slice [96, 28, 28, 2] -> [96, 16, 16, 2]"
    assert lines[11] == f"dwconv3x3 B=2 16x16 -> 16x16 C=96 pad=1 <- {BLOCK}.local_conv.c.weight"


def test_per_node_block_has_one_masked_attention(gguf):
    lines = _block_graph(gguf, False).describe().strip().splitlines()[:-1]
    assert [l for l in lines if l.startswith(("window_attention", "attention"))] == ["attention_masked B=8 heads=3 T=196 hd=32 mask=[3, 1] (constant)"], lines
    assert sum(l.startswith("heads_major") for l in lines) == 3 and sum(l.startswith("slice [32") for l in lines) == 3
    assert len(lines) == 16 + 7  # the q|k|v permute, three slices, three heads_major copies


def test_a_second_reader_of_q_keeps_the_per_node_form(gguf):
    """The match changes nothing unless every link is read by the next one only."""
    res, dim, _, heads, ws, _ = CFG.layers()[2]
    g = G.Graph(None, G.Weights(gguf))
    m = G.ModelRef(g, BLOCK)["attn"]
    x = g.input((dim, ws * ws, 4), G.F16, "x")
    q, k, v = G.split_qkv(m["qkv"], x, heads, 1)
    g.output(G.attention(m, q, k, v, m.weights("attention_biases_indexed"), 1.0 / np.sqrt(32.0), m["proj"]), "out")
    g.output(q, "q_too")
    g.allocate()
    lines = g.describe().splitlines()
    assert sum(l.startswith("attention_masked") for l in lines) == 1 and not any(l.startswith("window_attention") for l in lines)
    # ... and neither does another scale
    g2 = G.Graph(None, G.Weights(gguf))
    m2 = G.ModelRef(g2, BLOCK)["attn"]
    q, k, v = G.split_qkv(m2["qkv"], g2.input((dim, ws * ws, 4), G.F16, "x"), heads, 1)
    g2.output(G.attention(m2, q, k, v, m2.weights("attention_biases_indexed"), 0.25, m2["proj"]), "out")
    g2.allocate()
    assert not any(l.startswith("window_attention") for l in g2.describe().splitlines())


SWIN_BLOCK_LAUNCHES = """layer_norm rows=392 C=32
roll [32, 14, 14, 2] by [0, -3, -3, 0]
permute [224, 2, 7, 4] -> [224, 7, 2, 4]
pad_rows K=32->64 <- bb.layers.0.blocks.1.attn.qkv.weight
gemm M=392 N=96 K=32 <- bb.layers.0.blocks.1.attn.qkv.weight
permute [32, 1, 3, 392] -> [32, 1, 392, 3]
slice [32, 1, 392, 3] -> [32, 1, 392, 1]
slice [32, 1, 392, 3] -> [32, 1, 392, 1]
slice [32, 1, 392, 3] -> [32, 1, 392, 1]
heads_major q (scaled)
heads_major k
heads_major v
attention_masked B=8 heads=1 T=49 hd=32 mask=[1, 4] (constant)
pad_rows K=32->64 <- bb.layers.0.blocks.1.attn.proj.weight
gemm M=392 N=32 K=32 <- bb.layers.0.blocks.1.attn.proj.weight
permute [224, 7, 2, 4] -> [224, 2, 7, 4]
roll [32, 14, 14, 2] by [0, 3, 3, 0]
add n=12544 period=12544
layer_norm rows=392 C=32
pad_rows K=32->64 <- bb.layers.0.blocks.1.mlp.fc1.weight
gemm[gelu] M=392 N=128 K=32 <- bb.layers.0.blocks.1.mlp.fc1.weight
gemm[+res] M=392 N=32 K=128 <- bb.layers.0.blocks.1.mlp.fc2.weight
launches=22 nodes=56 buffers=23 arena_bytes=317952 unshared_bytes=833792 constant_bytes=66056
"""


def test_swin_block_plans_as_before(tmp_path):
    """SWIN splits q | k | v with split_dim 2 and carries a per-window mask: the launch list recorded before the window-attention match existed."""
    path = synth.write_swin_gguf(tmp_path / "mini.gguf", synth.SWIN_MINI, seed=5)
    g = G.Graph(None, G.Weights(path))
    m = G.ModelRef(g, "bb")
    G.swin_precompute(m, (56, 56), 7, 0)
    x = g.input((32, 196, 2), G.F16, "tokens")
    g.output(G.swin_block(m["layers"][0]["blocks"][1], x, g.get_tensor("swin_layer_14x14.attn_mask"), 1, 7, 14, 14, 3), "block")
    g.allocate()
    assert g.describe() == SWIN_BLOCK_LAUNCHES


def test_patch_embed_starts_with_image_pad8(gguf):
    g = G.Graph(None, G.Weights(gguf))
    img = g.input((3, 64, 48, 2), G.F32, "image")
    out = G.tinyvit_patch_embed(G.ModelRef(g, "enc.patch_embed"), img)
    assert out.ne == (32, 16, 12, 2)
    g.output(out, "out")
    g.allocate()
    assert g.describe().strip().splitlines()[:-1] == ["image_pad8 [3, 64, 48, 2]", "conv3x3s2[gelu] M=1536 N=16 K=72 <- enc.patch_embed.seq.0.c.weight",
                                                      "conv3x3s2 M=384 N=32 K=144 <- enc.patch_embed.seq.2.c.weight"]


def test_block_refuses_what_the_reference_asserts(gguf):
    g = G.Graph(None, G.Weights(gguf))
    m = G.ModelRef(g, BLOCK)
    with pytest.raises(ValueError, match="200 tokens do not form a 14x14 map"):
        G.tinyvit_block(m, g.input((96, 200, 1), G.F16, "a"), 14, 96, 3, 7)
    with pytest.raises(ValueError, match="one 14x14 window is not built"):
        G.tinyvit_block(m, g.input((96, 196, 1), G.F16, "b"), 14, 96, 3, 14)


@pytest.mark.parametrize("fused", [True, False])
def test_tinyvit_encode_of_the_mini_config_allocates(gguf, fused):
    g = G.Graph(None, G.Weights(gguf))
    m = G.ModelRef(g, "enc")
    out = G.tinyvit_encode(m, g.input((3, 256, 256, 2), G.F32, "image"), CFG.layers())
    assert out.ne == (256, 16, 16, 2)
    assert g.get_tensor("enc.patch_embed").ne == (32, 64, 64, 2) and g.get_tensor("enc.layers.0").ne == (64, 1024, 2, 1)
    assert g.get_tensor("enc.layers.2").ne == (320, 256, 2, 1) and g.get_tensor("enc.layers.3").ne == (320, 256, 2, 1)  # the last merging has stride 1
    g.output(out, "out")
    g.set_fused_models(fused)
    g.allocate()
    lines = g.describe().strip().splitlines()[:-1]
    blocks = sum(CFG.depths[1:])
    assert sum(l.startswith("window_attention" if fused else "attention_masked") for l in lines) == blocks
    assert sum(l.startswith("attention_masked" if fused else "window_attention") for l in lines) == 0
    assert sum(l.startswith("pad [") for l in lines) == blocks  # every windowed stage pads: 32 -> 35, 16 -> 28, 16 -> 21
    dw = [l for l in lines if l.startswith("dwconv")]
    assert len(dw) == CFG.depths[0] + 3 + blocks and sum(l.startswith("dwconv3x3s2") for l in dw) == 2
    assert lines[0] == "image_pad8 [3, 256, 256, 2]"


def test_cpp_face_builds_the_same_mb_conv_and_block(gguf):
    """tests/cpp/tinyvit_check.cpp: mb_conv and one tiny_vit_block through include/visp/nn.h, planned on the host; the launch lists equal the Python face's."""
    exe = Path(__file__).resolve().parents[1] / "vision.cpp_amd" / "lib" / "tinyvit_check"
    assert exe.exists(), "built by __graft_entry__.build()"
    res, dim, _, heads, ws, _ = CFG.layers()[2]
    for fused in (True, False):
        r = subprocess.run([str(exe), str(gguf), "block", BLOCK, str(dim), str(res), "2", str(heads), str(ws), str(int(fused))], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, (r.stdout, r.stderr)
        assert r.stdout == _block_graph(gguf, fused).describe()
        g = G.Graph(None, G.Weights(gguf))
        x = g.input((32, 20, 20, 2), G.F16, "x")
        g.output(G.tinyvit_mb_conv(G.ModelRef(g, "enc.layers.0.blocks.0"), x), "out")
        g.set_fused_models(fused)
        g.allocate()
        r = subprocess.run([str(exe), str(gguf), "mbconv", "enc.layers.0.blocks.0", "32", "20", "2", "0", "0", str(int(fused))], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, (r.stdout, r.stderr)
        if fused:
            assert [l.split()[0] for l in g.describe().strip().splitlines()[:-1]] == ["pad_rows", "gemm(conv1x1)[gelu]", "dwconv3x3[gelu]", "gemm(conv1x1)[+res]", "gelu"]
        assert r.stdout == g.describe()

"""The graph layer's image resize, image patches, pixel gate and in-place concat, and the BiRefNet builders of vision.cpp_amd/graph.py, without a GPU
(`Graph(None)`): shapes, every refusal by its message, the planned launch lists with fused models and per node, the whole birefnet_predict graph of
test_birefnet_every_level's setup (synth.SWIN_MINI at image_size 256, seed 6, 192 x 128, batch 2), and the C++ face (tests/cpp/birefnet_graph_check.cpp)
against the Python face.

One thing the graph layer still refuses: mul / add / sub of a map [C, W, H, N] and a per-image plane [1, W, H, N] with N > 1.
tests/test_graph_migan_cpu.py::test_plane_broadcast_refusals_name_both_forms pins that refusal for [1, 5, 3, 2] on [16, 5, 3, 2], so the gate of a decoder
level is built as mul(p, repeat(gate, p's shape)) at a batch above one (ggml_mul's broadcast written out). Both forms are one pixel_gate launch with fused
models; test_the_gate_plans_at_batch_2 holds the planned lists."""
import dataclasses
import subprocess
from pathlib import Path

import numpy as np
import pytest

from visioncpp_amd import _lib as L
from visioncpp_amd import graph as G
from visioncpp_amd import synth

ROOT = Path(__file__).resolve().parents[1]
CFG = dataclasses.replace(synth.SWIN_MINI, image_size=256)
W, H, B = 192, 128, 2


@pytest.fixture(scope="module")
def gguf(tmp_path_factory):
    return synth.write_birefnet_gguf(tmp_path_factory.mktemp("birefnet_graph") / "mini.gguf", CFG, seed=6)


def _lines(g):
    g.allocate()
    return g.describe().strip().splitlines()[:-1]


def _conv(g, name, cin, k, cout):
    g.add_weight(f"{name}.weight", np.zeros((cout, k, k, cin), np.float32), G.F16)
    g.add_weight(f"{name}.bias", np.zeros(cout, np.float32), G.F32)
    return G.ModelRef(g, name)


# ---- INTERPOLATE on an f32 image ------------------------------------------------------------------------------------------------------------------------

def test_image_resize_plans_and_every_image_reader_takes_it():
    g = G.Graph(None)
    m = G.ModelRef(g)
    image = g.input((3, W, H, B), G.F32, "image")
    half = G.birefnet_downscale_by(m, image, 2)  # interpolate(image, (96, 64), BILINEAR_AC)
    assert half.ne == (3, 96, 64, B) and half.dtype == G.F32
    quarter = G.interpolate(m, half, (48, 32), G.BILINEAR_AC)  # the result of this same op is a source too
    assert quarter.ne == (3, 48, 32, B) and quarter.dtype == G.F32
    g.add_weight("pe.proj.weight", np.zeros((32, 4, 4, 3), np.float32), G.F16)
    g.output(G.patch_embed(G.ModelRef(g, "pe"), half, 4), "tokens")
    g.output(G.conv_2d(_conv(g, "c3", 3, 3, 16), half, 2, 1), "conv")
    g.output(G.birefnet_image_to_patches(m, quarter, 12, 8), "patches")
    rgba = g.input((4, 24, 16, B), G.F32, "rgba")
    g.output(G.conv_2d(_conv(g, "c4", 4, 1, 16), G.interpolate(m, rgba, (12, 8), G.BILINEAR_AC)), "conv4")
    lines = _lines(g)
    assert lines[0] == "image_bilinear_ac 192x128 -> 96x64 C=3 B=2" and "image_bilinear_ac 96x64 -> 48x32 C=3 B=2" in lines and "image_bilinear_ac 24x16 -> 12x8 C=4 B=2" in lines
    assert "im2col_patches 4x4 M=768 <- tokens" in lines and "image_pad8 [3, 96, 64, 2]" in lines and "image4_pad8 [4, 12, 8, 2]" in lines
    assert "image_patches 48x32 -> 12x8 grid 4x4 C=3 -> 48 B=2" in lines


def test_image_resize_refusals_name_the_mode():
    g = G.Graph(None)
    m = G.ModelRef(g)
    image = g.input((3, 24, 16, B), G.F32, "image")
    for mode, words in ((G.SCALE_MODE_NEAREST, r"mode 0 \(nearest\)"), (G.SCALE_MODE_BILINEAR, r"mode 1 \(bilinear\)"), (G.SCALE_MODE_BICUBIC, r"mode 2 \(bicubic\)"),
                        (G.SCALE_MODE_BICUBIC | G.SCALE_FLAG_ALIGN_CORNERS, r"mode 258 \(bicubic \| align_corners\)")):
        with pytest.raises(L.Error, match=rf"^interpolate: {words} on an f32 image is not built \(bilinear \| align_corners is\)"):
            G.interpolate(m, image, (12, 8), mode)
    with pytest.raises(L.Error, match="interpolate: non-positive target extent"):
        G.interpolate(m, image, (0, 8), G.BILINEAR_AC)
    # what is no image stays refused as before: more than 4 channels, and an f32 map that something else computed
    with pytest.raises(L.Error, match="interpolate: operand 0 is f32; only patch_embed"):
        G.interpolate(m, g.input((5, 24, 16, B), G.F32, "five"), (12, 8), G.BILINEAR_AC)
    head = G.conv_2d(_conv(g, "head", 16, 1, 1), g.input((16, 24, 16, B), G.F16, "x"))
    assert head.dtype == G.F32
    with pytest.raises(L.Error, match="interpolate: operand 0 is f32; only patch_embed"):
        G.interpolate(m, head, (12, 8), G.BILINEAR_AC)
    # f16 maps are resized as before, in every mode they were
    assert G.interpolate(m, g.input((16, 24, 16, B), G.F16, "map"), (12, 8), G.BILINEAR_AC).dtype == G.F16


# ---- IMAGE_PATCHES ----------------------------------------------------------------------------------------------------------------------------------------

def test_image_patches_shape_plan_and_refusals():
    assert G.OP_IMAGE_PATCHES == 43
    g = G.Graph(None)
    m = G.ModelRef(g)
    image = g.input((3, W, H, B), G.F32, "image")
    p = G.birefnet_image_to_patches(m, image, 12, 8)
    assert p.ne == (16 * 16 * 3, 12, 8, B) and p.dtype == G.F16
    assert G.birefnet_image_to_patches(m, image, 24, 8).ne == (8 * 16 * 3, 24, 8, B)  # gw != gh
    with pytest.raises(L.Error, match=r"^image_patches: Grid must divide image size \(image 192x128, patches 13x8\)"):
        G.birefnet_image_to_patches(m, image, 13, 8)
    with pytest.raises(L.Error, match=r"^image_patches: Grid must divide image size"):
        G.birefnet_image_to_patches(m, image, 12, 7)
    with pytest.raises(L.Error, match=r"^image_patches: grid 1x1 of a 3-channel image gives 3 channels \(a multiple of 8; at grid 1 a conv reads the image itself\)"):
        G.birefnet_image_to_patches(m, image, W, H)
    with pytest.raises(L.Error, match=r"^image_patches: grid 2x2 of a 3-channel image gives 12 channels"):
        G.birefnet_image_to_patches(m, image, W // 2, H // 2)
    with pytest.raises(L.Error, match=r"^image_patches: the operand is an f32 image \[C <= 4, W, H, N\] .*not the f16 / integer tensor \[16, 24, 16, 2\]"):
        G.birefnet_image_to_patches(m, g.input((16, 24, 16, B), G.F16, "map"), 12, 8)
    with pytest.raises(L.Error, match=r"^image_patches: the operand is an f32 image .*not the f32 tensor \[5, 24, 16, 2\]"):
        G.birefnet_image_to_patches(m, g.input((5, 24, 16, B), G.F32, "five"), 12, 8)
    with pytest.raises(L.Error, match="image_patches: two positive integer parameters"):
        g.op(G.OP_IMAGE_PATCHES, [image], [12])
    with pytest.raises(L.Error, match="image_patches: takes 1..1 tensors"):
        g.op(G.OP_IMAGE_PATCHES, [image, image], [12, 8])
    # the reference's reshape / permute chain on the image (birefnet.cpp:158-160) stays refused: it lives in WHCN, which this layer keeps only as views
    with pytest.raises(L.Error, match="permute: operand 0 is f32"):
        G.permute(m, image, 0, 2, 1, 3)
    g.output(p, "patches")
    assert _lines(g) == ["image_patches 192x128 -> 12x8 grid 16x16 C=3 -> 768 B=2"]


# ---- the gate ------------------------------------------------------------------------------------------------------------------------------------------

def _gate(fused, batch, C=64, Cg=16):
    g = G.Graph(None)
    g.set_fused_models(fused)
    m = G.ModelRef(g)
    p, a = g.input((C, 12, 8, batch), G.F16, "p"), g.input((Cg, 12, 8, batch), G.F16, "a")
    gate = G.sigmoid(m, G.conv_2d(_conv(g, "attn", Cg, 1, 1), a))
    assert gate.ne == (1, 12, 8, batch)
    if batch > 1:
        gate = G.repeat(m, gate, *p.ne)
    g.output(G.mul(m, p, gate), "y")
    return g


def test_the_gate_plans_at_batch_2():
    assert _lines(_gate(True, 2)) == ["pixel_gate M=192 C=64 Cg=16 <- attn.weight"]
    assert _lines(_gate(False, 2)) == ["conv1x1_to_1 M=192 C=16 <- attn.weight", "sigmoid n=192", "repeat [1, 12, 8, 2] -> [64, 12, 8, 2]", "mul n=12288 period=12288"]
    # batch 1: the plane form that planned before, now one launch with fused models as well
    assert _lines(_gate(True, 1)) == ["pixel_gate M=96 C=64 Cg=16 <- attn.weight"]
    assert _lines(_gate(False, 1)) == ["conv1x1_to_1 M=96 C=16 <- attn.weight", "sigmoid n=96", "mul_plane B=1 HW=96 C=64"]
    assert _lines(_gate(True, 2, C=72, Cg=8)) == ["pixel_gate M=192 C=72 Cg=8 <- attn.weight"]


def test_a_gate_with_another_reader_is_not_fused():
    g = G.Graph(None)
    m = G.ModelRef(g)
    p, a = g.input((64, 12, 8, 2), G.F16, "p"), g.input((16, 12, 8, 2), G.F16, "a")
    gate = G.sigmoid(m, G.conv_2d(_conv(g, "attn", 16, 1, 1), a))
    g.output(gate, "gate")  # the gate itself is wanted: every link must be read by the next one only
    g.output(G.mul(m, p, G.repeat(m, gate, *p.ne)), "y")
    lines = _lines(g)
    assert not any(ln.startswith("pixel_gate") for ln in lines) and len(lines) == 4, lines


def test_a_per_image_plane_operand_is_still_refused():
    """[1, W, H, N] on [C, W, H, N] with N > 1: the refusal an existing test pins (see the module's docstring)."""
    g = G.Graph(None)
    m = G.ModelRef(g)
    p, a = g.input((64, 12, 8, 2), G.F16, "p"), g.input((16, 12, 8, 2), G.F16, "a")
    with pytest.raises(L.Error, match=r"mul: cannot broadcast \[1, 12, 8, 2\] onto \[64, 12, 8, 2\]"):
        G.mul(m, p, G.sigmoid(m, G.conv_2d(_conv(g, "attn", 16, 1, 1), a)))


# ---- swin_precompute twice --------------------------------------------------------------------------------------------------------------------------------

def test_swin_precompute_for_a_second_extent_finds_what_exists(gguf):
    g = G.Graph(None, G.Weights(gguf))
    m = G.ModelRef(g, "bb")
    full = G.swin_precompute(m, (W, H), CFG.window_size)
    half = G.swin_precompute(m, (W // 2, H // 2), CFG.window_size)
    assert half[0].index == full[0].index  # the relative position index: found, not added again
    assert [t.index for t in half[1:5]] == [t.index for t in full[2:6]]  # the half extent's masks are the full extent's, one level down
    assert half[5].index not in [t.index for t in full] and half[5].ne == (49, 49, 1, 1)  # ... and one more, for the 1 x 1 map
    assert [t.index for t in G.swin_precompute(m, (W, H), CFG.window_size)] == [t.index for t in full]  # a third call adds nothing
    g2 = G.Graph(None, G.Weights(gguf))
    G.birefnet_precompute(G.ModelRef(g2), (W, H), CFG.window_size)
    assert g2.get_tensor("swin_layer_24x16.attn_mask") is not None and g2.get_tensor("swin_layer_1x1.attn_mask") is not None


# ---- encode_concat -------------------------------------------------------------------------------------------------------------------------------------------

FEATURES = [(32, 48, 32), (64, 24, 16), (128, 12, 8), (256, 6, 4)]  # SWIN_MINI at 192 x 128: (C, w, h) of the four stages; the half-size pass gives half the extents


def _encode_concat(fused, device=None):
    g = G.Graph(device)
    g.set_fused_models(fused)
    m = G.ModelRef(g)
    xs = [g.input((c, w, h, B), G.F16, f"xs{i}") for i, (c, w, h) in enumerate(FEATURES)]
    xs_low = [g.input((c, w // 2, h // 2, B), G.F16, f"xs_low{i}") for i, (c, w, h) in enumerate(FEATURES)]
    outs = [g.output(t, f"feature_{i}") for i, t in enumerate(G.birefnet_encode_concat(m, xs, xs_low))]
    return g, xs, xs_low, outs


def test_encode_concat_is_written_in_place():
    g, _, _, outs = _encode_concat(False)
    assert [t.ne for t in outs] == [(64, 48, 32, B), (128, 24, 16, B), (256, 12, 8, B), (960, 6, 4, B)]
    per_node = _lines(g)
    assert sum(ln.startswith("bilinear_ac ") for ln in per_node) == 7 and sum(ln.startswith("concat part") for ln in per_node) == 14 and len(per_node) == 21
    fused = _lines(_encode_concat(True)[0])
    resizes = [ln for ln in fused if ln.startswith("bilinear_ac[out ch ")]
    copies = [ln for ln in fused if ln.startswith("concat part")]
    print(f"encode_concat on graph inputs: {len(per_node)} launches per node, {len(fused)} with fused models ({len(resizes)} resizes into place + {len(copies)} copies of the inputs)")
    # every resize writes its slice; what is left are the copies of the four maps that were there before the concat (graph inputs here: nothing writes them)
    assert len(resizes) == 7 and len(copies) == 4 and len(fused) == 11, fused
    assert "bilinear_ac[out ch 192..448 of 960] 12x8 -> 6x4 C=256" in fused and "bilinear_ac[out ch 704..960 of 960] 3x2 -> 6x4 C=256" in fused
    assert "concat part 3 [256, 6, 4, 2] -> [960, 6, 4, 2]" in fused  # the left-folded five-way concat is ONE buffer: its fourth part is copied once, not three times


def test_a_resize_from_one_pixel_and_a_decoder_block_keep_their_plan(gguf):
    """bilinear | align_corners from a 1 x 1 source is a broadcast and is not placed: aspp_deformable's concat (birefnet.cpp:127-132) plans as before."""
    g = G.Graph(None, G.Weights(gguf))
    xi = g.input((960, 6, 4, 1), G.F16, "feature_3")
    g.output(G.birefnet_basic_decoder_block(G.ModelRef(g, "squeeze_module.0"), xi), "squeeze")
    lines = _lines(g)
    assert sum(ln.startswith("bilinear_ac 1x1 -> 6x4") for ln in lines) == 1 and not any(ln.startswith("bilinear_ac[") for ln in lines)
    assert sum(ln.startswith("concat part") for ln in lines) == 8


# ---- the whole graph ---------------------------------------------------------------------------------------------------------------------------------------

def _predict(gguf, fused, device=None, captures=True):
    g = G.Graph(device, G.Weights(gguf))
    g.set_fused_models(fused)
    m = G.ModelRef(g)
    image = g.input((3, W, H, B), G.F32, "image")
    G.birefnet_precompute(m, (W, H), CFG.window_size)
    out = G.birefnet_predict(m, image, CFG.window_size, CFG.depths, CFG.n_heads, captures=captures)
    return g, image, out


def test_the_whole_graph_plans_in_both_modes(gguf):
    inside = set(ln for ln in _lines(_encode_concat(False)[0]) if ln.startswith("concat part"))  # encode_concat's own copies, by their text
    assert len(inside) == 14
    plans = {}
    for fused in (True, False):
        g, image, out = _predict(gguf, fused)
        assert out.ne == (1, W, H, B)
        for name, ne in (("feature_0", (64, 48, 32, B)), ("feature_3", (960, 6, 4, B)), ("squeeze", (512, 6, 4, B)), ("p4", (256, 6, 4, B)), ("p3", (128, 12, 8, B)),
                         ("p2", (64, 24, 16, B)), ("p1", (32, 48, 32, B))):
            assert g.get_tensor(name).ne == ne, name
        plans[fused] = _lines(g)
    fused, per_node = plans[True], plans[False]
    print(f"birefnet_predict, SWIN_MINI 192 x 128 batch 2: {len(fused)} launches with fused models, {len(per_node)} per node")
    assert len(fused) < len(per_node)
    assert [ln for ln in fused if ln.startswith("pixel_gate")] == ["pixel_gate M=48 C=256 Cg=16 <- decoder.gdt_convs_attn_4.0.weight", "pixel_gate M=192 C=128 Cg=16 <- decoder.gdt_convs_attn_3.0.weight",
                                                                    "pixel_gate M=768 C=64 Cg=16 <- decoder.gdt_convs_attn_2.0.weight"]  # one per gated level
    assert not any(ln.startswith("pixel_gate") for ln in per_node) and sum(ln.startswith("repeat [1, ") for ln in per_node) == 3
    assert inside <= set(per_node) and not inside & set(fused)  # no copy inside encode_concat: the resizes and the encoder's last LayerNorms write the slices
    assert sum(ln.startswith("bilinear_ac[out ch ") for ln in fused) == 8 and sum(ln.startswith("layer_norm[out ch ") for ln in fused) == 4  # (the eighth: _p1 into conv_out1's input)
    for lines in plans.values():
        assert lines.count("image_bilinear_ac 192x128 -> 96x64 C=3 B=2") == 1 and sum(ln.startswith("image_patches 192x128") for ln in lines) == 4
        assert sum(ln.startswith("bilinear_ac 1x1 -> ") for ln in lines) == 5  # the five decoder blocks as they plan on their own
    # without the captures nothing moves in either mode but the arena
    assert _lines(_predict(gguf, True, captures=False)[0]) == fused


def test_cpp_face_builds_the_same_level(gguf):
    """tests/cpp/birefnet_graph_check.cpp: the image resize, patches, simple_conv, the concat and the gate through include/visp/nn.h, planned on the host."""
    exe = ROOT / "vision.cpp_amd" / "lib" / "birefnet_graph_check"
    assert exe.exists(), "built by __graft_entry__.build()"
    for fused in (True, False):
        for batch in (1, 2):
            g = G.Graph(None, G.Weights(gguf))
            g.set_fused_models(fused)
            m = G.ModelRef(g)
            dec = m["decoder"]
            image, carried = g.input((3, W, H, batch), G.F32, "image"), g.input((256, W // 16, H // 16, batch), G.F16, "p3_in")
            half = G.birefnet_downscale_by(m, image, 2)
            patches = G.birefnet_simple_conv(dec["ipt_blk4"], G.birefnet_image_to_patches(m, image, carried.ne[1], carried.ne[2]))
            half_patches = G.birefnet_image_to_patches(m, half, carried.ne[1], carried.ne[2])
            x = G.concat(m, [carried, patches], 0)
            x = G.relu(m, G.conv_2d(dec["block3"]["conv_in"], x, 1, 1))
            x = G.conv_2d(dec["block3"]["conv_out"], x, 1, 1)
            gate = G.sigmoid(m, G.conv_2d(dec["gdt_convs_attn_3.0"], G.birefnet_gdt_conv(dec["gdt_convs_3"], x)))
            g.output(G.mul(m, x, G.repeat(m, gate, *x.ne) if batch > 1 else gate), "p3")
            g.output(half_patches, "half_patches")
            g.allocate()
            r = subprocess.run([str(exe), str(gguf), str(W), str(H), str(batch), str(int(fused))], capture_output=True, text=True, timeout=120)
            assert r.returncode == 0, (r.stdout, r.stderr)
            assert r.stdout == g.describe(), (fused, batch)
            assert ("pixel_gate M=" in r.stdout) == fused

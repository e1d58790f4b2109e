"""Small graphs at the edges of the executor's fusion patterns, built the same way by the planning tests (tests/test_graph_cpu.py, `Graph(None)`)
and by the GPU tests that check their numbers (tests/test_gpu_graph_ops.py). Weights are rounded to f16 where the executor holds them in f16,
so the numpy / torch references see the same operands."""
from __future__ import annotations

import math

import numpy as np

from visioncpp_amd import graph as G
from visioncpp_amd import synth


def h(a):
    return np.asarray(a, np.float32).astype(np.float16).astype(np.float32)


def conv_weight(g, name, rng, cout, cin, k=3, bias=True):
    """OHWI weight [cout, k, k, cin] (+ f32 bias); returns the host arrays."""
    w = h(rng.standard_normal((cout, k, k, cin)) / math.sqrt(k * k * cin))
    g.add_weight(f"{name}.weight", w)
    b = None
    if bias:
        b = (0.1 * rng.standard_normal(cout)).astype(np.float32)
        g.add_weight(f"{name}.bias", b, G.F32)
    return w, b


def conv_relu_add(g, rng, cout, W=20, H=18, B=2):
    """conv3x3 (Cin 64 -> cout, stride 1, pad 1) -> relu -> + another map: the LDS-ring conv's shape with an add its epilogue cannot take."""
    m = G.ModelRef(g)
    w, b = conv_weight(g, "c", rng, cout, 64)
    x = g.input((64, W, H, B), G.F16, "x")
    o = g.input((cout, W, H, B), G.F16, "other")
    y = g.output(G.add(m, G.relu(m, G.conv_2d(m["c"], x, 1, 1)), o), "y")
    return {"x": x, "other": o, "y": y, "w": w, "b": b}


def residual_unit_on_planes(g, rng, W=20, H=18, B=2):
    """x0 = conv3x3(f32 image -> 64) lives as planes of the LDS-ring conv; then relu -> conv64 -> relu -> conv64 -> + x0 (dpt::residual_conv's
    shape, depth-anything.cpp:15-23) with the planar map as its skip operand."""
    m = G.ModelRef(g)
    w0, b0 = conv_weight(g, "c0", rng, 64, 3)
    w1, b1 = conv_weight(g, "c1", rng, 64, 64)
    w2, b2 = conv_weight(g, "c2", rng, 64, 64)
    img = g.input((3, W, H, B), G.F32, "image")
    x0 = G.conv_2d(m["c0"], img, 1, 1)
    o = G.conv_2d(m["c1"], G.relu(m, x0), 1, 1)
    o = G.conv_2d(m["c2"], G.relu(m, o), 1, 1)
    y = g.output(G.add(m, x0, o), "y")
    return {"image": img, "y": y, "w": [(w0, b0), (w1, b1), (w2, b2)]}


def relu_into_output_conv(g, rng, planar, W=20, H=18, B=2):
    """relu -> conv3x3 64 -> 64 whose result is a graph output, on an NHWC input map or on the planes of a first conv of the f32 image (which
    has a second reader, so the relu is not that conv's epilogue)."""
    m = G.ModelRef(g)
    w1, b1 = conv_weight(g, "c1", rng, 64, 64)
    out = {}
    if planar:
        w0, b0 = conv_weight(g, "c0", rng, 64, 3)
        src = g.input((3, W, H, B), G.F32, "image")
        x = G.conv_2d(m["c0"], src, 1, 1)
        out["x0"] = g.output(x, "x0")
        out["w0"] = (w0, b0)
    else:
        src = x = g.input((64, W, H, B), G.F16, "x")
    out.update(src=src, y=g.output(G.conv_2d(m["c1"], G.relu(m, x), 1, 1), "y"), w1=(w1, b1))
    return out


def conv_leaky(g, rng, slope, W=20, H=18, B=2):
    """conv3x3 64 -> 64 -> leaky_relu(slope): only slope 0.2 is an epilogue of the LDS-ring conv."""
    m = G.ModelRef(g)
    w, b = conv_weight(g, "c", rng, 64, 64)
    x = g.input((64, W, H, B), G.F16, "x")
    y = g.output(G.leaky_relu(m, G.conv_2d(m["c"], x, 1, 1), slope), "y")
    return {"x": x, "y": y, "w": w, "b": b}


def conv_narrow_input(g, rng, cin, cout=32, W=20, H=18, B=2):
    """conv3x3 (cin 16 or 48 -> 32, stride 1, pad 1) on a 20-wide NHWC map: the LDS-ring conv's output widths and map size with an input narrower
    than its 32-channel pixel stride (16: the GEMM family's conv) or no multiple of its chunk (48: run as 64 with zero weights)."""
    m = G.ModelRef(g)
    w, b = conv_weight(g, "c", rng, cout, cin)
    x = g.input((cin, W, H, B), G.F16, "x")
    y = g.output(G.conv_2d(m["c"], x, 1, 1), "y")
    return {"x": x, "y": y, "w": w, "b": b}


def encoder_chain(g, rng, scales, ps=14, side=2, B=2):
    """dino::prepare_tokens (dino.cpp:32-46) and len(scales) encoder layers of width 384 / MLP 1536 / 6 heads written out like dino_layer
    (dino.cpp:48-90), each attention with its own explicit scale; the last residual stream goes through a final LayerNorm (a tap) to the output."""
    D, HID, NH = 384, 1536, 6
    T = side * side + 1
    m = G.ModelRef(g)
    w = {}

    def lin(name, n, k):
        w[f"{name}.weight"] = h(rng.standard_normal((n, k)) / math.sqrt(k))
        w[f"{name}.bias"] = (0.05 * rng.standard_normal(n)).astype(np.float32)

    w["e.patch_embeddings.projection.weight"] = h(rng.standard_normal((D, ps, ps, 3)) / math.sqrt(ps * ps * 3))
    w["e.patch_embeddings.projection.bias"] = (0.1 * rng.standard_normal(D)).astype(np.float32)
    w["e.cls_token"] = rng.standard_normal((1, 1, D)).astype(np.float32)
    w["e.position_embeddings"] = rng.standard_normal((1, T, D)).astype(np.float32)
    for i in range(len(scales)):
        p = f"l.{i}"
        for nm in ("norm1", "norm2", "final"):
            w[f"{p}.{nm}.weight"] = (1 + 0.1 * rng.standard_normal(D)).astype(np.float32)
            w[f"{p}.{nm}.bias"] = (0.1 * rng.standard_normal(D)).astype(np.float32)
        for nm in ("query", "key", "value", "dense"):
            lin(f"{p}.{nm}", D, D)
        lin(f"{p}.fc1", HID, D)
        lin(f"{p}.fc2", D, HID)
        w[f"{p}.ls1.lambda1"] = (0.5 + 0.1 * rng.standard_normal(D)).astype(np.float32)
        w[f"{p}.ls2.lambda1"] = (0.5 + 0.1 * rng.standard_normal(D)).astype(np.float32)
    for k, v in w.items():
        g.add_weight(k, v, G.F16 if v.ndim == 2 or v.ndim == 4 else G.F32)
    img = g.input((3, side * ps, side * ps, B), G.F32, "image")
    x = G.dino_prepare_tokens(m["e"], img, ps)
    for i, s in enumerate(scales):
        L = m["l"][i]
        att = G.layer_norm(L["norm1"], x, 1e-6)
        q, k, v = (G.reshape(m, G.linear(L[nm], att), D // NH, NH, T, B) for nm in ("query", "key", "value"))
        att = G.attention(L, q, k, v, None, s, L["dense"])
        x = G.add(m, x, G.mul(m, att, L["ls1"].weights("lambda1")))
        f = G.linear(L["fc2"], G.gelu(m, G.linear(L["fc1"], G.layer_norm(L["norm2"], x, 1e-6))))
        x = G.add(m, x, G.mul(m, f, L["ls2"].weights("lambda1")))
    last = m["l"][len(scales) - 1]
    y = g.output(G.layer_norm(last["final"], x, 1e-6), "y")
    return {"image": img, "y": y}


# ---- one aspp_module_deformable (birefnet.cpp:109-114): the planning tests, the C++ face and tools/lowering_fingerprint.py build the same module

DEFORM_C_IN, DEFORM_PLANES, DEFORM_KERNEL, DEFORM_W, DEFORM_H, DEFORM_B = 64, 256, 3, 13, 9, 2


def deform_module_weights(seed=3):
    """name -> (numpy array in torch order of the graph layer's layout, dtype): kernels [Cout, kh, kw, Cin]"""
    rng = np.random.default_rng(seed)
    t = DEFORM_KERNEL * DEFORM_KERNEL
    out = {}
    for name, co, bias in (("offset", 2 * t, True), ("modulator", t, True), ("conv", DEFORM_PLANES, False)):
        out[f"aspp.conv.{name}.weight"] = ((rng.standard_normal((co, DEFORM_KERNEL, DEFORM_KERNEL, DEFORM_C_IN)) * 0.05).astype(np.float32), G.F16)
        if bias:
            out[f"aspp.conv.{name}.bias"] = ((rng.standard_normal(co) * 0.05).astype(np.float32), G.F32)
    out["aspp.bn.weight"] = ((1 + 0.1 * rng.standard_normal(DEFORM_PLANES)).astype(np.float32), G.F32)
    out["aspp.bn.bias"] = ((0.1 * rng.standard_normal(DEFORM_PLANES)).astype(np.float32), G.F32)
    return out


def deform_module(g, add_weights=True):
    """The module on a [64, 13, 9, 2] map; `add_weights` False: the graph was made on a file that holds them."""
    if add_weights:
        for name, (a, dt) in deform_module_weights().items():
            g.add_weight(name, a, dt)
    x = g.input((DEFORM_C_IN, DEFORM_W, DEFORM_H, DEFORM_B), G.F16, "x")
    y = g.output(G.birefnet_aspp_module_deformable(G.ModelRef(g, "aspp"), x, DEFORM_KERNEL // 2), "branch")
    return {"x": x, "y": y}


# ---- SWIN_MINI (graphs made on the file synth.write_swin_gguf(path, synth.SWIN_MINI, seed=5) writes)

def swin_block_mini(g):
    """bb.layers.0.blocks.1 of SWIN_MINI (C = 32, one head, shift 3) on a 14 x 14 map, two images."""
    m = G.ModelRef(g, "bb")
    G.swin_precompute(m, (56, 56), 7, 0)
    x = g.input((32, 196, 2), G.F16, "tokens")
    y = g.output(G.swin_block(m["layers"][0]["blocks"][1], x, g.get_tensor("swin_layer_14x14.attn_mask"), 1, 7, 14, 14, 3), "block")
    return {"x": x, "y": y}


def swin_encode_mini(g):
    """swin_encode of SWIN_MINI at 256 x 288 (maps 64x72 .. 8x9: every stage pads)."""
    cfg = synth.SWIN_MINI
    m = G.ModelRef(g, "bb")
    image = g.input((3, 256, 288, 2), G.F32, "image")
    G.swin_precompute(m, (256, 288), cfg.window_size)
    outs = G.swin_encode(m, image, cfg.window_size, cfg.depths, cfg.n_heads)
    return {"image": image, "outs": [g.output(o, f"out{i}") for i, o in enumerate(outs)]}

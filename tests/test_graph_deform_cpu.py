"""The graph layer's deformable conv, sigmoid and mean_2d without a GPU (`Graph(None)`): shape inference against numpy, host folding of sigmoid
on a constant, every refusal by its message, batch_norm_2d's refusal, the planned launch list of one aspp_module_deformable
(birefnet.cpp:109-114) with and without fused models, and the C++ face (tests/cpp/deform_check.cpp) against the Python face."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import deform_ref as R
import graph_cases as GC
from visioncpp_amd import _lib as L
from visioncpp_amd import graph as G


def _kernel(g, name, cout, k, cin, kh=None):
    return g.add_weight(name, np.zeros((cout, kh or k, k, cin), np.float32))


def test_shape_inference_of_the_three_ops_follows_numpy():
    g = G.Graph(None)
    m = G.ModelRef(g)
    B, h, w, C = 2, 5, 7, 16
    x = g.input((C, w, h, B), G.F16, "x")
    xa = np.zeros((B, h, w, C))
    for i, (k, pad, cout) in enumerate([(1, 0, 32), (3, 1, 48), (7, 3, 256), (3, 0, 8), (3, 2, 8)]):
        oh, ow = h + 2 * pad - k + 1, w + 2 * pad - k + 1
        want = R.deform_conv2d(xa, np.zeros((cout, k, k, C)), np.zeros((B, oh, ow, 2 * k * k)), None, pad).shape
        off = g.input((2 * k * k, ow, oh, B), G.F16, f"off{i}")
        mask = g.input((k * k, ow, oh, B), G.F16, f"mask{i}")
        wt = _kernel(g, f"w{i}", cout, k, C)
        for t in (G.conv_2d_deform(m, x, wt, off, None, 1, pad), G.conv_2d_deform(m, x, wt, off, mask, 1, pad)):
            assert t.ne == want[::-1] and t.dtype == G.F16 and not t.is_constant, (k, pad)
    assert G.sigmoid(m, x).ne == x.ne and G.sigmoid(m, x).dtype == G.F16
    assert G.mean_2d(m, x).ne == R.mean_2d(xa).shape[::-1] == (C, 1, 1, B)


def test_sigmoid_of_a_constant_is_folded_on_the_host():
    g = G.Graph(None)
    m = G.ModelRef(g)
    a = np.linspace(-12, 12, 2 * 3 * 5).reshape(2, 3, 5).astype(np.float32)
    s = G.sigmoid(m, g.add_weight("c", a, G.F32))
    assert s.is_constant and s.ne == (5, 3, 2, 1)
    np.testing.assert_allclose(g.read_constant(s)[0], R.sigmoid(a), rtol=1e-6)
    twice = G.scale(m, s, 2.0)  # ... and what is computed from it
    assert twice.is_constant
    np.testing.assert_allclose(g.read_constant(twice)[0], 2 * R.sigmoid(a), rtol=1e-6)


def test_refusals_name_the_op():
    g = G.Graph(None)
    m = G.ModelRef(g)
    x = g.input((16, 7, 5, 2), G.F16, "x")
    off3 = g.input((18, 7, 5, 2), G.F16, "off3")
    mask3 = g.input((9, 7, 5, 2), G.F16, "mask3")
    w3 = _kernel(g, "w3", 32, 3, 16)
    with pytest.raises(L.Error, match="conv_2d_deform: stride 2 is not built"):
        G.conv_2d_deform(m, x, w3, off3, mask3, 2, 1)
    with pytest.raises(L.Error, match="conv_2d_deform: kernel 3x1; square kernels only"):
        G.conv_2d_deform(m, x, _kernel(g, "w31", 32, 3, 16, kh=1), off3, mask3, 1, 1)
    x24 = g.input((24, 7, 5, 2), G.F16, "x24")
    with pytest.raises(L.Error, match="conv_2d_deform: Cin = 24 must be a multiple of 16"):
        G.conv_2d_deform(m, x24, _kernel(g, "w24", 32, 3, 24), off3, mask3, 1, 1)
    with pytest.raises(L.Error, match="conv_2d_deform: Cout = 264; one block computes every output channel of its pixels, at most 256"):
        G.conv_2d_deform(m, x, _kernel(g, "wbig", 264, 3, 16), off3, mask3, 1, 1)
    with pytest.raises(L.Error, match=r"conv_2d_deform: offset \[9, 7, 5, 2\] does not match a 3x3 kernel on a 7x5 output"):
        G.conv_2d_deform(m, x, w3, mask3, None, 1, 1)
    with pytest.raises(L.Error, match=r"conv_2d_deform: offset \[18, 7, 5, 2\] does not match a 3x3 kernel on a 5x3 output"):
        G.conv_2d_deform(m, x, w3, off3, None, 1, 0)  # the output extent without padding is 5 x 3
    with pytest.raises(L.Error, match=r"conv_2d_deform: mask \[18, 7, 5, 2\] does not match a 3x3 kernel on a 7x5 output"):
        G.conv_2d_deform(m, x, w3, off3, off3, 1, 1)
    with pytest.raises(L.Error, match=r"conv_2d_deform: mask \[9, 7, 5, 1\] does not match"):
        G.conv_2d_deform(m, x, w3, off3, g.input((9, 7, 5, 1), G.F16, "mask_b1"), 1, 1)
    with pytest.raises(L.Error, match="conv_2d_deform: the kernel must be a model weight"):
        G.conv_2d_deform(m, x, g.input((16, 3, 3, 32), G.F16, "w_act"), off3, mask3, 1, 1)
    with pytest.raises(L.Error, match="conv_2d_deform: kernel .* does not match input"):
        G.conv_2d_deform(m, x, _kernel(g, "w32in", 32, 3, 32), off3, mask3, 1, 1)


def test_batch_norm_2d_refuses_unfused_statistics():
    g = G.Graph(None)
    x = g.input((8, 4, 4, 1), G.F16, "x")
    for n in ("weight", "bias"):
        g.add_weight(f"ok.{n}", np.ones(8, np.float32), G.F32)
        g.add_weight(f"bad.{n}", np.ones(8, np.float32), G.F32)
    g.add_weight("bad.running_var", np.ones(8, np.float32), G.F32)
    y = G.batch_norm_2d(G.ModelRef(g, "ok"), x)
    assert y.ne == x.ne
    with pytest.raises(ValueError, match="Batch norm was not fused"):
        G.batch_norm_2d(G.ModelRef(g, "bad"), x)


# ---- the planned launch list of one aspp_module_deformable ----------------------------------------------------------------------------------

C_IN, PLANES, KERNEL, W, H, B = GC.DEFORM_C_IN, GC.DEFORM_PLANES, GC.DEFORM_KERNEL, GC.DEFORM_W, GC.DEFORM_H, GC.DEFORM_B
_module_weights = GC.deform_module_weights


def _module_graph(fused: bool, weights=None):
    g = G.Graph(None, weights)
    GC.deform_module(g, add_weights=weights is None)
    g.set_fused_models(fused)
    g.allocate()
    return g


def test_fused_models_plan_two_launches_for_the_module():
    lines = _module_graph(True).describe().strip().splitlines()[:-1]
    M, K = B * H * W, KERNEL * KERNEL * C_IN
    assert lines == [f"deform_offsets conv3x3 M={M} N=27 K={K} <- aspp.conv.offset.weight",
                     f"deform_conv[logits x2][*scale][+bias][relu] M={M} N={PLANES} K={K} k=3 <- aspp.conv.conv.weight"], lines
    assert not [l for l in lines if l.startswith(("sigmoid", "scale", "mul", "add", "relu"))]


def test_without_fused_models_every_node_is_a_launch():
    lines = _module_graph(False).describe().strip().splitlines()[:-1]
    M, K = B * H * W, KERNEL * KERNEL * C_IN
    n = M * PLANES
    # (a conv whose channel count is no multiple of 8 -- 18 offsets, 9 logits -- writes rows padded to 8 and compacts them with one copy)
    nodes = [l for l in lines if not l.startswith("unpad_rows")]
    assert nodes == [f"conv3x3 M={M} N=18 K={K} <- aspp.conv.offset.weight", f"conv3x3 M={M} N=9 K={K} <- aspp.conv.modulator.weight",
                     f"sigmoid n={M * 9}", f"scale n={M * 9}", f"deform_conv[mask] M={M} N={PLANES} K={K} k=3 <- aspp.conv.conv.weight",
                     f"mul n={n} period={PLANES} (constant)", f"add n={n} period={PLANES} (constant)", f"relu n={n}"], lines
    assert [l for l in lines if l.startswith("unpad_rows")] == ["unpad_rows N=24->18 <- aspp.conv.offset.weight", "unpad_rows N=16->9 <- aspp.conv.modulator.weight"]


def test_any_other_use_of_the_op_takes_the_generic_form():
    """The same module with the offsets read by a second node too: no group, the deformable conv reads offsets and mask where they are."""
    g = G.Graph(None)
    for name, (a, dt) in _module_weights().items():
        g.add_weight(name, a, dt)
    m = G.ModelRef(g, "aspp.conv")
    x = g.input((C_IN, W, H, B), G.F16, "x")
    offset = G.conv_2d(m["offset"], x, 1, 1)
    mask = G.scale(m, G.sigmoid(m, G.conv_2d(m["modulator"], x, 1, 1)), 2.0)
    g.output(G.conv_2d_deform(m, x, m.weights("conv.weight"), offset, mask, 1, 1), "y")
    g.output(G.scale(m, offset, 0.5), "offsets_too")
    g.allocate()
    lines = g.describe().splitlines()
    assert not [l for l in lines if l.startswith("deform_offsets")] and len([l for l in lines if l.startswith("deform_conv[mask]")]) == 1, lines
    # a deformable conv without a mask, offsets a constant
    g2 = G.Graph(None)
    w = _kernel(g2, "w", 32, 3, 16)
    y = G.conv_2d_deform(G.ModelRef(g2), g2.input((16, 7, 5, 2), G.F16, "x"), w, g2.add_weight("off", np.zeros((2, 5, 7, 18), np.float32)), None, 1, 1)
    g2.output(y, "y")
    g2.allocate()
    assert g2.describe().splitlines()[0] == "deform_conv M=70 N=32 K=144 k=3 <- w"


def test_cpp_face_builds_the_same_module(tmp_path):
    """tests/cpp/deform_check.cpp: the module through include/visp/nn.h with VISP_GGML_NAMES, planned on the host; its launch lists equal the Python face's."""
    from visioncpp_amd.gguf import GGUFWriter

    path = tmp_path / "aspp.gguf"
    wr = GGUFWriter(path, "birefnet")
    wr.add_string("birefnet.tensor_data_layout", "cwhn")
    for name, (a, dt) in _module_weights().items():
        wr.add_tensor(name, a.astype(np.float16) if dt == G.F16 else a)
    wr.write()
    exe = Path(__file__).resolve().parents[1] / "vision.cpp_amd" / "lib" / "deform_check"
    assert exe.exists(), "built by __graft_entry__.build()"
    for fused in (True, False):
        g = _module_graph(fused, G.Weights(path))
        r = subprocess.run([str(exe), str(path), "aspp", str(C_IN), str(W), str(H), str(B), str(KERNEL // 2), str(int(fused))], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, (r.stdout, r.stderr)
        assert r.stdout == g.describe()
        assert g.describe() == _module_graph(fused).describe()  # weights from a file or added by hand: the same plan

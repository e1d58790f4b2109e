"""The graph layer's attention_cross, mul_mat, sin and cos ops and the SAM prompt-encoder / mask-decoder builders without a GPU (`Graph(None)`): shape
inference against numpy, host folding, every refusal by its message, the refusals of OP_ATTENTION and OP_ATTENTION_MASKED that must stay, the planned
launch lists of sam_decoder_attention, embed_points / embed_box, one two-way block and the whole sam_predict_masks (dim 256, mlp 256, a 12 x 12
embedding) with fused models and per node, recorded as they come out, and the C++ face (tests/cpp/samdec_check.cpp) against the Python face."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import cross_attn_ref as R
from visioncpp_amd import _lib as L
from visioncpp_amd import graph as G
from visioncpp_amd import synth

ROOT = Path(__file__).resolve().parents[1]
DIM, MLP, SIDE = 256, 256, 12


@pytest.fixture(scope="module")
def gguf(tmp_path_factory):
    return synth.write_sam_decoder_gguf(tmp_path_factory.mktemp("samdec") / "dec12.gguf", synth.sam_decoder_state_dict(11, mlp_dim=MLP), SIDE)


def _lines(g):
    return g.describe().strip().splitlines()[:-1]


def _new(path, fused):
    g = G.Graph(None, G.Weights(path))
    g.set_fused_models(fused)
    return g, G.ModelRef(g)


# ---- the ops -----------------------------------------------------------------------------------------------------------------------------------------

def test_op_values_and_shapes():
    assert (G.OP_ATTENTION_CROSS, G.OP_MUL_MAT, G.OP_SIN, G.OP_COS) == (38, 39, 40, 41)
    g = G.Graph(None)
    m = G.ModelRef(g)
    for hd, H, Tq, Tk, B, _ in R.ATTENTION_CASES:
        q, k, v = (g.input((hd, H, T, B), G.F16, f"{n}{hd}{H}{Tq}{Tk}{B}") for n, T in (("q", Tq), ("k", Tk), ("v", Tk)))
        x = g.op(G.OP_ATTENTION_CROSS, [q, k, v], fparams=[hd ** -0.5])
        want = R.attention(*R.attention_operands((hd, H, Tq, Tk, B, 1.0)), hd ** -0.5)
        assert x.ne[:3] == want.shape[::-1] and x.ne[3] == 1 and x.dtype == G.F16 and not x.is_constant
    for K, M, N, B, Ba in R.MUL_MAT_CASES:
        a, b = g.input((K, M, Ba), G.F16, f"a{K}{M}{N}{B}"), g.input((K, N, B), G.F16, f"b{K}{M}{N}{B}")
        y = G.mul_mat(m, a, b)
        assert y.ne[:3] == R.mul_mat(np.zeros((Ba, M, K)), np.zeros((B, N, K))).shape[::-1] and y.dtype == G.F16
    x = g.input((1003, 3, 2), G.F16, "x")
    assert G.sin(m, x).ne == x.ne and G.cos(m, x).ne == x.ne and G.sin(m, x).dtype == G.F16


def test_constants_are_folded():
    g = G.Graph(None)
    m = G.ModelRef(g)
    rng = np.random.default_rng(0)
    a, b = rng.standard_normal((1, 5, 12)).astype(np.float32), rng.standard_normal((2, 17, 12)).astype(np.float32)  # K = 12, N = 17: no device limits on constants
    y = G.mul_mat(m, g.add_weight("a", a, G.F32), g.add_weight("b", b, G.F32))
    assert y.is_constant and y.ne == (5, 17, 2, 1)
    np.testing.assert_allclose(g.read_constant(y)[0], R.mul_mat(a, b), rtol=1e-6, atol=1e-6)
    v = np.linspace(-20, 20, 41).astype(np.float32)
    c = g.add_weight("v", v, G.F32)
    np.testing.assert_array_equal(g.read_constant(G.sin(m, c)).ravel(), np.sin(v.astype(np.float64)).astype(np.float32))
    np.testing.assert_array_equal(g.read_constant(G.cos(m, c)).ravel(), np.cos(v.astype(np.float64)).astype(np.float32))


def test_attention_cross_refusals():
    g = G.Graph(None)
    m = G.ModelRef(g)

    def qkv(hd, Tq, Tk, Tv=None, dtype=G.F16, name=""):
        return [g.input((hd, 2, T, 1), dt, f"{n}{name}") for n, T, dt in (("q", Tq, dtype), ("k", Tk, G.F16), ("v", Tv or Tk, G.F16))]

    with pytest.raises(L.Error, match=r"^attention_cross: head_dim 48; the kernel is built for head_dim 16, 32 and 64"):
        g.op(G.OP_ATTENTION_CROSS, qkv(48, 7, 9, name="a"), fparams=[1.0])
    with pytest.raises(L.Error, match=r"^attention_cross: q \[16, 2, 7, 1\], k \[16, 2, 9, 1\], v \[16, 2, 10, 1\] do not match"):
        g.op(G.OP_ATTENTION_CROSS, qkv(16, 7, 9, 10, name="b"), fparams=[1.0])
    with pytest.raises(L.Error, match=r"^attention_cross: operand 0 \(q\) is f32; q, k and v are f16 activations"):
        g.op(G.OP_ATTENTION_CROSS, qkv(16, 7, 9, dtype=G.F32, name="c"), fparams=[1.0])
    q, k, v = qkv(16, 7, 9, name="d")
    with pytest.raises(L.Error, match=r"^attention_cross: operand 1 \(k\) is a constant"):
        g.op(G.OP_ATTENTION_CROSS, [q, g.add_weight("kc", np.zeros((1, 9, 2, 16), np.float32)), v], fparams=[1.0])
    with pytest.raises(L.Error, match=r"^attention_cross: takes 3..3 tensors"):
        g.op(G.OP_ATTENTION_CROSS, [q, k], fparams=[1.0])
    assert G.attention_cross(m, q, k, v, 0.25, _Lin(g, 32, 24)).ne == (24, 7, 1, 1)


class _Lin(G.ModelRef):
    """a linear layer's weights under a fresh prefix"""
    count = 0

    def __init__(self, g, k, n):
        _Lin.count += 1
        super().__init__(g, f"lin{_Lin.count}")
        g.add_weight(f"{self.prefix}.weight", np.zeros((n, k), np.float32))


def test_mul_mat_refusals():
    g = G.Graph(None)
    m = G.ModelRef(g)
    act = lambda ne, name, dt=G.F16: g.input(ne, dt, name)
    with pytest.raises(L.Error, match=r"^mul_mat: K = 12; two activations are multiplied for K a multiple of 8, at most 256"):
        G.mul_mat(m, act((12, 5, 1), "a1"), act((12, 4, 1), "b1"))
    with pytest.raises(L.Error, match=r"^mul_mat: K = 264; two activations"):
        G.mul_mat(m, act((264, 5, 1), "a2"), act((264, 4, 1), "b2"))
    with pytest.raises(L.Error, match=r"^mul_mat: N = 17 columns in the second operand; at most 16"):
        G.mul_mat(m, act((32, 5, 1), "a3"), act((32, 17, 1), "b3"))
    with pytest.raises(L.Error, match=r"^mul_mat: the first operand's batch 3 is neither 1 nor the second's 2"):
        G.mul_mat(m, act((32, 5, 3), "a4"), act((32, 4, 2), "b4"))
    with pytest.raises(L.Error, match=r"^mul_mat: a \[32, 5, 1, 1\] and b \[24, 4, 1, 1\] do not match"):
        G.mul_mat(m, act((32, 5, 1), "a5"), act((24, 4, 1), "b5"))
    with pytest.raises(L.Error, match=r"^mul_mat: operands of two activations are f16 \(a is f16, b is f32\)"):
        G.mul_mat(m, act((32, 5, 1), "a6"), act((32, 4, 1), "b6", G.F32))
    const = lambda shape, name: g.add_weight(name, np.ones(shape, np.float32))
    # a constant first operand: LINEAR is the op, and the message says so
    with pytest.raises(L.Error, match=r"^mul_mat: the first operand is a constant; use LINEAR"):
        G.mul_mat(m, const((5, 32), "w1"), act((32, 4, 1), "b7"))
    with pytest.raises(L.Error, match=r"^mul_mat: the second operand is a constant and the first an activation.*LINEAR"):
        G.mul_mat(m, act((32, 5, 1), "a8"), const((4, 32), "w2"))
    # K = 2: on an f32 graph input only ...
    with pytest.raises(L.Error, match=r"^mul_mat: a constant first operand with K = 2 is built on an f32 graph input only .* not on an f16 activation"):
        G.mul_mat(m, const((128, 2), "g1"), act((2, 3, 1), "c16"))
    # ... and there only as the head of the Fourier chain: refused when the graph is lowered
    y = G.mul_mat(m, const((128, 2), "g2"), act((2, 3, 1), "c32", G.F32))
    assert y.ne == (128, 3, 1, 1)
    g.output(G.relu(m, y), "y")
    with pytest.raises(L.Error, match=r"^mul_mat: a constant first operand with K = 2 on f32 coordinates is built as the head of mul_mat -> scale\(2 pi\) -> \{sin, cos\} -> concat"):
        g.allocate()


def test_a_chain_with_another_scale_is_not_the_fourier_group():
    g = G.Graph(None)
    m = G.ModelRef(g)
    t = G.scale(m, G.mul_mat(m, g.add_weight("g", np.ones((8, 2), np.float32)), g.input((2, 3, 1), G.F32, "c")), 3.0)
    g.output(G.concat(m, [G.sin(m, t), G.cos(m, t)], 0), "y")
    with pytest.raises(L.Error, match=r"^mul_mat: a constant first operand with K = 2 on f32 coordinates is built as the head"):
        g.allocate()


def test_attention_and_attention_masked_keep_their_refusals():
    g = G.Graph(None)
    m = G.ModelRef(g)
    q, k, v = (g.input((32, 2, 9, 1), G.F16, n) for n in "qkv")
    g.output(g.op(G.OP_ATTENTION, [q, k, v], fparams=[1.0]), "y")
    with pytest.raises(L.Error, match=r"^attention: head_dim 32, 9 queries on 9 keys; the fused kernel is built for head_dim 64 self-attention"):
        g.allocate()
    g = G.Graph(None)
    q = g.input((32, 2, 7, 1), G.F16, "q")
    k, v = (g.input((32, 2, 9, 1), G.F16, n) for n in "kv")
    with pytest.raises(L.Error, match=r"^attention_masked: 7 queries on 9 keys; cross-attention \(T_q != T_k\) is not built"):
        g.op(G.OP_ATTENTION_MASKED, [q, k, v, g.input((9, 7, 1, 1), G.F16, "mask")], fparams=[1.0])
    q, k, v = (g.input((16, 2, 9, 1), G.F16, n + "16") for n in "qkv")
    with pytest.raises(L.Error, match=r"^attention_masked: head_dim 16; the masked kernel is built for head_dim 32 and 64"):
        g.op(G.OP_ATTENTION_MASKED, [q, k, v, g.input((9, 9, 1, 1), G.F16, "mask16")], fparams=[1.0])
    # the builder: mask = None is OP_ATTENTION, a mask OP_ATTENTION_MASKED, as before
    g = G.Graph(None)
    m = G.ModelRef(g)
    q, k, v = (g.input((64, 2, 9, 1), G.F16, n) for n in "qkv")
    g.output(G.attention(m, q, k, v, None, 0.125, _Lin(g, 128, 128)), "y")
    g.allocate()
    assert [ln.split()[0] for ln in _lines(g)] == ["heads_major", "heads_major", "heads_major", "attention", "gemm"]


# ---- launch lists ----------------------------------------------------------------------------------------------------------------------------------------

def test_decoder_attention_is_three_products_one_attention_one_product(gguf):
    for fused in (True, False):
        g, m = _new(gguf, fused)
        q, k = g.input((DIM, 7, 1), G.F16, "q"), g.input((DIM, 144, 1), G.F16, "k")
        g.output(G.sam_decoder_attention(m["dec.transformer.layers.0.cross_attn_t2i"], q, k, k, 8), "y")
        g.allocate()
        p = "dec.transformer.layers.0.cross_attn_t2i"
        assert _lines(g) == [f"gemm M=7 N=128 K=256 <- {p}.q_proj.weight", f"gemm M=144 N=128 K=256 <- {p}.k_proj.weight", f"gemm M=144 N=128 K=256 <- {p}.v_proj.weight",
                             "attention_cross B=1 heads=8 Tq=7 Tk=144 hd=16", f"gemm M=7 N=256 K=128 <- {p}.out_proj.weight"]


def test_split_keys_are_two_listed_launches():
    g = G.Graph(None)
    q = g.input((16, 8, 7, 1), G.F16, "q")
    k, v = (g.input((16, 8, 4096, 1), G.F16, n) for n in "kv")
    g.output(g.op(G.OP_ATTENTION_CROSS, [q, k, v], fparams=[0.25]), "y")
    g.allocate()
    assert _lines(g) == ["attention_cross B=1 heads=8 Tq=7 Tk=4096 hd=16 parts=32", "attention_cross_combine B=1 heads=8 Tq=7 parts=32 hd=16"]


def test_prompt_embeddings_are_one_fourier_launch(gguf):
    for fused in (True, False):
        g, m = _new(gguf, fused)
        g.output(G.sam_embed_points(m["prompt_encoder"], g.input((2, 2, 1), G.F32, "coords")), "points")
        g.allocate()
        assert _lines(g) == ["fourier_features points=2 F=128 <- prompt_encoder.pe_layer.positional_encoding_gaussian_matrix", "slice [256, 2, 1, 1] -> [256, 1, 1, 1]", "add n=256 period=256 (constant)",
                             "concat part 0 [256, 1, 1, 1] -> [256, 2, 1, 1]", "concat part 1 [256, 1, 1, 1] -> [256, 2, 1, 1] (constant)"]
        g, m = _new(gguf, fused)
        g.output(G.sam_embed_box(m["prompt_encoder"], g.input((2, 2, 1), G.F32, "coords")), "box")
        g.allocate()
        assert _lines(g) == ["fourier_features points=2 F=128 <- prompt_encoder.pe_layer.positional_encoding_gaussian_matrix", "slice [256, 2, 1, 1] -> [256, 1, 1, 1]", "add n=256 period=256 (constant)",
                             "slice [256, 2, 1, 1] -> [256, 1, 1, 1]", "add n=256 period=256 (constant)", "concat part 0 [256, 1, 1, 1] -> [256, 2, 1, 1]",
                             "concat part 1 [256, 1, 1, 1] -> [256, 2, 1, 1]"]
        assert not any(ln.startswith(("gemm", "mul_mat", "sin", "cos", "scale")) for ln in _lines(g))


def _block(path, fused, n=7, batch=1):
    g, m = _new(path, fused)
    tokens, token_pe = g.input((DIM, n, batch), G.F16, "tokens"), g.input((DIM, n, batch), G.F16, "token_pe")
    keys, key_pe = g.input((DIM, SIDE * SIDE, batch), G.F16, "map"), g.input((DIM, SIDE * SIDE, batch), G.F16, "map_pe")
    qs, ks = G.sam_two_way_attention_block(m["dec.transformer.layers.1"], tokens, keys, token_pe, key_pe, 8, False)
    g.output(qs, "queries")
    g.output(ks, "keys")
    g.allocate()
    return g


BLOCK_KINDS = ["add", "gemm", "gemm", "gemm", "attention_cross", "gemm[+res]", "layer_norm", "add", "add", "gemm", "gemm", "gemm", "attention_cross", "gemm[+res]", "layer_norm",
               "gemm[relu]", "gemm[+res]", "layer_norm", "add", "gemm", "gemm", "gemm", "attention_cross", "gemm[+res]", "layer_norm"]


def test_two_way_block(gguf):
    for fused in (True, False):
        lines = _lines(_block(gguf, fused))
        assert [ln.split()[0] for ln in lines] == BLOCK_KINDS
        assert [ln for ln in lines if ln.startswith("attention_cross")] == ["attention_cross B=1 heads=8 Tq=7 Tk=7 hd=32", "attention_cross B=1 heads=8 Tq=7 Tk=144 hd=16",
                                                                            "attention_cross B=1 heads=8 Tq=144 Tk=7 hd=16"]


def _masks(path, fused, n=2, batch=1):
    g, m = _new(path, fused)
    embed, prompt = g.input((DIM, SIDE, SIDE, 1), G.F16, "embed"), g.input((DIM, n, batch), G.F16, "prompt")
    masks, iou = G.sam_predict_mask(m, embed, prompt)
    g.allocate()
    return g, masks, iou


def test_predict_masks_launch_lists(gguf):
    counts = {}
    for fused in (True, False):
        g, masks, iou = _masks(gguf, fused)
        assert masks.ne == (4 * SIDE, 4 * SIDE, 4, 1) and iou.ne == (4, 1, 1, 1)
        lines = _lines(g)
        counts[fused] = len(lines)
        assert sum(ln.startswith("attention_cross ") for ln in lines) == 7
        assert not any(ln.startswith("heads_major") for ln in lines)
        assert [ln for ln in lines if ln.startswith("mul_mat")] == ["mul_mat M=2304 N=4 K=32 B=1"]
        assert not any(ln.startswith("repeat") for ln in lines)  # batch 1: the repeat of the embedding to its own shape is a view
        # fused: the four hypernetwork MLPs and the iou head read their token row in place (gemm[rows i.. of n]); per node: five slice copies more
        assert sum(ln.startswith("slice") for ln in lines) == (1 if fused else 6)
    assert counts == {True: 89, False: 94}
    # two prompts are batch entries: the embedding is repeated by one copy launch, every attention runs at B = 2
    lines = _lines(_masks(gguf, True, batch=2)[0])
    assert "repeat [256, 12, 12, 1] -> [256, 12, 12, 2]" in lines and "attention_cross B=2 heads=8 Tq=144 Tk=7 hd=16" in lines and "mul_mat M=2304 N=4 K=32 B=2" in lines


def test_cpp_face_builds_the_same_block_and_decoder(gguf):
    """tests/cpp/samdec_check.cpp: one two_way_attention_block and predict_masks through include/visp/nn.h, planned on the host; the launch lists equal the Python face's."""
    exe = ROOT / "vision.cpp_amd" / "lib" / "samdec_check"
    assert exe.exists(), "built by __graft_entry__.build()"
    for fused in (True, False):
        for batch in (1, 2):
            r = subprocess.run([str(exe), str(gguf), "block", str(DIM), str(SIDE), "7", str(batch), str(int(fused))], capture_output=True, text=True, timeout=120)
            assert r.returncode == 0, (r.stdout, r.stderr)
            assert r.stdout == _block(gguf, fused, 7, batch).describe()
            r = subprocess.run([str(exe), str(gguf), "masks", str(DIM), str(SIDE), "2", str(batch), str(int(fused))], capture_output=True, text=True, timeout=120)
            assert r.returncode == 0, (r.stdout, r.stderr)
            assert r.stdout == _masks(gguf, fused, 2, batch)[0].describe()

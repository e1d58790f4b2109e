"""The reference of tests/relpos_attn_ref.py pinned to transformers' SamVisionAttention in float64 (bias indices, the unscaled-q convention), the condition
that makes the GPU test sensitive to a dropped bias, and the refusals of the ATTENTION_REL_POS node through the graph API. No GPU."""
import numpy as np
import pytest
import torch
from transformers import SamVisionConfig
from transformers.models.sam.modeling_sam import SamVisionAttention

import relpos_attn_ref as R
from visioncpp_amd import graph as G


@pytest.mark.parametrize("gw, gh", [(4, 4), (5, 3)], ids=["square", "non_square"])
def test_reference_is_sam_vision_attention(gw, gh):
    """q, k, v are HF's own (its qkv linear, unrounded), the output linear is the identity: the reference's `want` is the module's output. The module takes
    its softmax in float32 whatever the dtype of the model, so the two agree to a few f32 roundings of weights that sum to 1 (1e-6 of outputs below 1); a
    wrong index, axis or a scaled q in the bias moves the output by a tenth."""
    heads, B = 2, 2
    torch.manual_seed(gw)
    attn = SamVisionAttention(SamVisionConfig(hidden_size=heads * R.HD, num_attention_heads=heads, image_size=64, patch_size=16), window_size=0).double().eval()
    with torch.no_grad():
        attn.rel_pos_h = torch.nn.Parameter(torch.randn(2 * gh - 1, R.HD, dtype=torch.float64) * 0.25)
        attn.rel_pos_w = torch.nn.Parameter(torch.randn(2 * gw - 1, R.HD, dtype=torch.float64) * 0.25)
        attn.proj.weight.copy_(torch.eye(heads * R.HD))
        attn.proj.bias.zero_()
        x = torch.randn(B, gh, gw, heads * R.HD, dtype=torch.float64)
        want = attn(x)[0].reshape(B * gw * gh, heads * R.HD).numpy()
        q, k, v = attn.qkv(x).reshape(B, gw * gh, 3, heads, R.HD).unbind(2)
    a = dict(q=q.numpy(), k=k.numpy(), v=v.numpy(), rel_h=attn.rel_pos_h.detach().numpy(), rel_w=attn.rel_pos_w.detach().numpy(), B=B, H=heads, gw=gw, gh=gh,
             scale=np.float32(attn.scale))
    got, _, written = R.evaluate_relpos(a)
    assert written.all() and np.abs(want).max() < 1.5 and np.abs(got - want).max() < 1e-6


@pytest.mark.parametrize("case", R.CASES, ids=[str(c) for c in R.CASES])
def test_a_dropped_bias_is_outside_the_allowance(case):
    a = R.operands(case)
    want, allow, _ = R.evaluate_relpos(a, guard_rows=32)
    assert (allow[-32:] == 0).all() and (allow[:-32] > 0).all()
    if case[0] * case[1] > 1:  # a single token's softmax is 1 whatever the bias
        assert (np.abs(R.evaluate_relpos(a, guard_rows=32, with_bias=False)[0] - want) > allow).any()


def _node(hd=64, heads=2, gw=3, gh=5, T=None, rows_h=None, rows_w=None, q_dtype=G.F16, k_tokens=None):
    g = G.Graph(None)
    m = G.ModelRef(g)
    T = gw * gh if T is None else T
    g.add_weight("rel_pos_h", np.zeros((2 * gh - 1 if rows_h is None else rows_h, hd), np.float32))
    g.add_weight("rel_pos_w", np.zeros((2 * gw - 1 if rows_w is None else rows_w, hd), np.float32))
    g.add_weight("proj.weight", np.zeros((hd * heads, hd * heads), np.float32))
    q = g.input((hd, heads, T, 1), q_dtype, "q")
    k, v = (g.input((hd, heads, T if k_tokens is None else k_tokens, 1), G.F16, name) for name in "kv")
    return G.attention_rel_pos(m, q, k, v, gw, gh, 0.125, m["proj"])


REFUSALS = [(dict(hd=80), "head_dim 80"), (dict(hd=80), "ViT-H's 80 is out of scope"), (dict(T=16), "16 tokens on a 3 x 5 grid"), (dict(gw=65, gh=1), "gw and gh are 1..64"),
            (dict(gw=0, gh=1, T=1, rows_w=1), "gw and gh are 1..64"), (dict(rows_h=11), "rel_h has 11 rows, a grid of 5 needs 2 g - 1 = 9"),
            (dict(rows_w=3), "rel_w has 3 rows, a grid of 3 needs 2 g - 1 = 5"), (dict(q_dtype=G.F32), "q, k and v are f16 activations"), (dict(k_tokens=16), "do not match")]


@pytest.mark.parametrize("fields, message", REFUSALS, ids=[m for _, m in REFUSALS])
def test_node_refusals(fields, message):
    assert _node().ne == (128, 15, 1, 1)
    with pytest.raises(Exception, match=message.replace("(", r"\(").replace(")", r"\)")):
        _node(**fields)

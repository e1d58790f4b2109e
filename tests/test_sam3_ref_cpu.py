"""tests/sam3_ref.py pinned: the float64 reference of the SAM3 encoders against `transformers`, and the numpy emulations of vx_rope_f16 / vx_get_rows_f16
against the allowance the GPU tests use (tests/test_gpu_graph_sam3.py). No GPU.

torch and transformers (with models.sam3) are preconditions of these tests: they are imported plainly, and a test fails where they are missing or have
changed. transformers' SAM3 modules are imported as the plain module (importlib): its lazy attribute face asks for torchvision, which the layer, embedding,
neck and rotary classes do not use.

Measured distances (largest absolute difference over largest reference value; torch runs f32, so all of it is torch's rounding):
  rope vs Sam3ViTRotaryEmbedding + apply_rotary_pos_emb_2d   5.3e-8 .. 6.2e-8  (3x3 and 5x3 positions, scales 1, 0.5, 1/3)
  Sam3ViTLayer window 4 / global, 8x8 and 6x6 (padded)       5.0e-7 .. 7.4e-7
  Sam3ViTEmbeddings tiled 4x4 -> 8x8 / untiled                1.3e-7, 1.5e-7
  Sam3VisionNeck hidden states / position encodings          2.8e-7 .. 5.0e-7 / 1.6e-7 .. 4.3e-7
  Sam3SinePositionEmbedding normalised / not                  3.2e-7, 1.1e-7
  CLIPTextModel 2 layers, 8 tokens, padded causal mask        5.2e-7"""
from __future__ import annotations

import importlib
import math

import numpy as np
import pytest

import torch
import transformers  # noqa: F401  (a precondition: nothing here skips)

import sam3_ref as R
from visioncpp_amd import synth

MODULE_BOUND = 1e-4  # of the largest reference value; the expected distance is near 1e-6 (torch runs f32), a convention error is of order 1


def _sam3_modeling():
    return importlib.import_module("transformers.models.sam3.modeling_sam3")  # the plain module: a failure here fails the test


def _dist(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    d = float(np.abs(got - want).max() / np.abs(want).max())
    print(f"distance {d:.3g}")
    return d


def _vit_config(cfg: synth.Sam3VitConfig, grid: int):
    from transformers.models.sam3.configuration_sam3 import Sam3ViTConfig
    return Sam3ViTConfig(hidden_size=cfg.hidden, intermediate_size=cfg.mlp, num_hidden_layers=cfg.n_layers, num_attention_heads=cfg.heads, image_size=grid * cfg.patch,
                         patch_size=cfg.patch, window_size=cfg.window, pretrain_image_size=cfg.pretrain_grid * cfg.patch, global_attn_indexes=list(cfg.global_layers),
                         hidden_act="gelu_pytorch_tanh", layer_norm_eps=1e-5)


def _load(module, w, prefix):
    sd = {k: torch.from_numpy(np.asarray(w[f"{prefix}.{k}"], np.float32)) for k in module.state_dict().keys()}
    module.load_state_dict(sd)
    return module.eval()


# ---- against transformers ------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("end_x, end_y", [(3, 3), (5, 3)])
@pytest.mark.parametrize("scale", [1.0, 0.5, 1.0 / 3.0])
def test_rope_matches_transformers(end_x, end_y, scale):
    """rope_2d against Sam3ViTRotaryEmbedding + apply_rotary_pos_emb_2d; bound 1e-5 of the largest value."""
    M = _sam3_modeling()
    cfg = _vit_config(synth.SAM3_VIT_MINI, 8)
    cos, sin = M.Sam3ViTRotaryEmbedding(cfg, end_x=end_x, end_y=end_y, scale=scale)()
    rng = np.random.default_rng(3)
    T, hd = end_x * end_y, cfg.hidden_size // cfg.num_attention_heads
    q = rng.standard_normal((2, cfg.num_attention_heads, T, hd)).astype(np.float32)  # transformers: [B, heads, T, hd]
    want, _ = M.apply_rotary_pos_emb_2d(torch.from_numpy(q), torch.from_numpy(q), cos=cos, sin=sin)
    px, py = np.arange(T) % end_x, np.arange(T) // end_x
    got = R.rope_2d(q.transpose(0, 2, 1, 3), px, py, 10000.0, scale)
    assert _dist(got.transpose(0, 2, 1, 3), want.numpy()) < 1e-5


@pytest.mark.parametrize("window, grid", [(4, 8), (0, 8), (4, 6), (0, 6)])
def test_vision_layer_matches_transformers(window, grid):
    M = _sam3_modeling()
    cfg = synth.SAM3_VIT_MINI
    w = {k: v for k, v in synth.sam3_vision_state_dict(cfg, 2, prefix="").items()}
    layer = _load(M.Sam3ViTLayer(_vit_config(cfg, grid), window_size=window), w, "backbone.layers.0")
    x = np.random.default_rng(4).standard_normal((2, grid, grid, cfg.hidden)).astype(np.float32)
    with torch.no_grad():
        want = layer(torch.from_numpy(x)).numpy()
    n = window if window else grid
    px, py = R.rope_2d_positions(n * n, n)
    got = R.vision_layer(w, "backbone.layers.0", x.astype(np.float64), window, cfg.heads, (px, py, 1.0 if window else cfg.window / grid))
    assert _dist(got, want) < MODULE_BOUND


@pytest.mark.parametrize("grid", [8, 4])  # pretrain 4x4 tiled to 8x8, and the untiled case
def test_vision_embed_matches_transformers(grid):
    M = _sam3_modeling()
    cfg = synth.SAM3_VIT_MINI
    sd = synth.sam3_vision_state_dict(cfg, 2, prefix="")
    emb = _load(M.Sam3ViTEmbeddings(_vit_config(cfg, grid)), sd, "backbone.embeddings")
    img = np.random.default_rng(5).standard_normal((2, 3, grid * cfg.patch, grid * cfg.patch)).astype(np.float32)
    with torch.no_grad():
        want = emb(torch.from_numpy(img)).numpy()  # [B, T, C]
    w = dict(sd)
    w["backbone.embeddings.patch_embeddings.projection.weight"] = sd["backbone.embeddings.patch_embeddings.projection.weight"].transpose(0, 2, 3, 1)
    got = R.vision_embed(w, "backbone.embeddings", img.transpose(0, 2, 3, 1), cfg.patch)
    assert _dist(got.reshape(want.shape), want) < MODULE_BOUND


def test_vision_neck_matches_transformers():
    M = _sam3_modeling()
    from transformers.models.sam3.configuration_sam3 import Sam3VisionConfig
    cfg = synth.SAM3_VIT_MINI
    sd = synth.sam3_vision_state_dict(cfg, 2, prefix="")
    neck = M.Sam3VisionNeck(Sam3VisionConfig(backbone_config=_vit_config(cfg, 8), fpn_hidden_size=cfg.fpn_dim, scale_factors=[4.0, 2.0, 1.0, 0.5]))
    neck.fpn_layers[0].scale_layers[1] = torch.nn.GELU(approximate="tanh")  # ggml_gelu is the tanh form (the reference's own test compares at 1e-2 instead)
    neck = _load(neck, sd, "neck")
    x = np.random.default_rng(6).standard_normal((2, cfg.hidden, 8, 8)).astype(np.float32)
    with torch.no_grad():
        want_h, want_p = neck(torch.from_numpy(x))
    w = {k: (v.transpose(0, 2, 3, 1) if v.ndim == 4 and "scale_layers" not in k else v) for k, v in sd.items()}
    got_h, got_p = R.vision_neck(w, "neck", x.transpose(0, 2, 3, 1).astype(np.float64))
    for i in range(4):
        assert _dist(got_h[i], want_h[i].numpy().transpose(0, 2, 3, 1)) < MODULE_BOUND, i
        assert _dist(got_p[i], want_p[i].numpy().transpose(0, 2, 3, 1)[0]) < MODULE_BOUND, i


@pytest.mark.parametrize("normalize", [True, False])
def test_sine_position_embedding_matches_transformers(normalize):
    M = _sam3_modeling()
    want = M.Sam3SinePositionEmbedding(num_position_features=16, normalize=normalize)(torch.Size((1, 32, 6, 10)), "cpu", torch.float32).numpy()
    got = R.sine_position_embedding(10, 6, 16, normalize)
    assert _dist(got, want[0].transpose(1, 2, 0)) < MODULE_BOUND


def _clip_inputs(cfg, n_tokens=5, batch=2):
    rng = np.random.default_rng(7)
    ids = rng.integers(1, cfg.vocab - 1, (batch, cfg.positions))
    ids[:, 0], ids[:, n_tokens - 1:] = 0, cfg.vocab - 1  # bos, then eos and padding
    from visioncpp_amd import graph as G
    return ids, G.clip_causal_mask(n_tokens, cfg.positions)


def test_clip_text_encoder_matches_transformers():
    """CLIPTextModel, 2 layers, 8 tokens, the causal mask with padding rows as clip_tokenizer::tokenize builds it. Measured: 5.2e-7."""
    from transformers import CLIPTextConfig, CLIPTextModel
    cfg = synth.CLIP_TEXT_MINI
    sd = synth.clip_text_state_dict(cfg, 3, prefix="")
    hf = CLIPTextModel(CLIPTextConfig(vocab_size=cfg.vocab, hidden_size=cfg.hidden, intermediate_size=cfg.mlp, num_hidden_layers=cfg.n_layers, num_attention_heads=cfg.heads,
                                      max_position_embeddings=cfg.positions, hidden_act="gelu_pytorch_tanh", bos_token_id=0, eos_token_id=cfg.vocab - 1, pad_token_id=cfg.vocab - 1,
                                      attn_implementation="eager"))
    tm = hf.text_model if hasattr(hf, "text_model") else hf  # (flat since transformers 5)
    state = {k: torch.from_numpy(sd["text_encoder.text_model." + k]) for k in tm.state_dict().keys() if "position_ids" not in k}
    tm.load_state_dict(state, strict=False)
    tm.eval()
    ids, mask = _clip_inputs(cfg)
    # the mask enters transformers as its 4-D additive form ([B, 1, T, T], taken as it is): causal rows for the prompt, the padding rows see the whole prompt
    mask4 = torch.from_numpy(np.where(np.isinf(mask), np.finfo(np.float32).min, 0.0).astype(np.float32))[None, None].expand(ids.shape[0], 1, -1, -1)
    with torch.no_grad():
        enc = tm.encoder(inputs_embeds=tm.embeddings(input_ids=torch.from_numpy(ids)), attention_mask=mask4)
        want = tm.final_layer_norm(enc.last_hidden_state).numpy()
    got = R.clip_encode_text(sd, "text_encoder.text_model", ids, mask.astype(np.float64), cfg.heads)
    d = _dist(got, want)
    assert d < MODULE_BOUND
    assert d < 1e-5, "above the f32 noise of torch: find out why before using the bound's slack"


def test_clip_mask_is_the_tokenizers():
    """sam3.h:146-192: row r < n sees keys 0..r, the padding rows see the n tokens of the prompt."""
    from visioncpp_amd import graph as G
    m = G.clip_causal_mask(3, 5)
    want = np.array([[0, 1, 1, 1, 1], [0, 0, 1, 1, 1], [0, 0, 0, 1, 1], [0, 0, 0, 1, 1], [0, 0, 0, 1, 1]], bool)
    assert np.array_equal(np.isinf(m), want) and m.dtype == np.float16 and (m[~want] == 0).all()


# ---- the kernel emulations against the allowance of the GPU tests -------------------------------------------------------------------------------------------------

def _halves(case):
    _, hd, heads, T, B, (px, py), scale = case
    return hd // 2, (px, py), scale


@pytest.mark.parametrize("case", R.ROPE_CASES, ids=[c[0] for c in R.ROPE_CASES])
@pytest.mark.parametrize("q_scale", [1.0, R.VX_ATTN_Q_SCALE])
def test_kernel_emulation_is_inside_the_allowance(case, q_scale):
    n, pos, scale = _halves(case)
    q, _ = R.rope_case_data(case)
    for h in range(2):
        x = q[..., h * n:(h + 1) * n]
        ref = R.rope(x.astype(np.float64), pos[h], n, R.ROPE_BASE, scale) * q_scale
        got = R.emulate_rope_kernel(x, R.rope_table(pos[h], n, R.ROPE_BASE, scale), q_scale).astype(np.float64)
        excess = np.abs(got - ref) - R.rope_allowance(ref, x, q_scale)
        assert excess.max() <= 0, (case[0], h, float(excess.max()))


WRONG = ["halves_swapped", "rotate_half", "sin_sign", "scale_dropped", "x_table_for_both", "i_over_n"]


@pytest.mark.parametrize("wrong", WRONG)
def test_modelled_wrong_kernels_fall_outside_the_allowance(wrong):
    """Each convention error moves many elements by far more than the allowance, on a case where it can show (positions that differ in x and y, a scale != 1)."""
    case = R.ROPE_CASES[5]  # arbitrary positions at scale 1 / 3
    _, hd, heads, T, B, (px, py), scale = case
    n = hd // 2
    q, _ = R.rope_case_data(case)
    ref = R.rope_2d(q.astype(np.float64), px, py, R.ROPE_BASE, scale)
    tx, ty = R.rope_table(px, n, R.ROPE_BASE, scale), R.rope_table(py, n, R.ROPE_BASE, scale)
    variant = wrong if wrong in ("rotate_half", "sin_sign") else ""
    if wrong == "halves_swapped":
        tx, ty = ty, tx
    elif wrong == "scale_dropped":
        tx, ty = R.rope_table(px, n, R.ROPE_BASE, 1.0), R.rope_table(py, n, R.ROPE_BASE, 1.0)
    elif wrong == "x_table_for_both":
        ty = tx
    elif wrong == "i_over_n":  # base^(-i / n): the table of twice the width has these frequencies in its first half of each part
        def half_freq(pos):
            th = np.asarray(pos, np.float64)[:, None] * (scale * np.power(R.ROPE_BASE, -np.arange(n // 2) / n))[None, :]
            return np.concatenate([np.cos(th), np.sin(th)], 1).astype(np.float32)
        tx, ty = half_freq(px), half_freq(py)
    got = np.concatenate([R.emulate_rope_kernel(q[..., :n], tx, 1.0, variant), R.emulate_rope_kernel(q[..., n:], ty, 1.0, variant)], -1).astype(np.float64)
    outside = np.abs(got - ref) > R.rope_allowance(ref, q, 1.0)
    assert outside.mean() > 0.25, (wrong, float(outside.mean()))
    right = np.concatenate([R.emulate_rope_kernel(q[..., :n], R.rope_table(px, n, R.ROPE_BASE, scale)), R.emulate_rope_kernel(q[..., n:], R.rope_table(py, n, R.ROPE_BASE, scale))], -1)
    assert not (np.abs(right.astype(np.float64) - ref) > R.rope_allowance(ref, q, 1.0)).any()


def test_get_rows_emulation_zeroes_out_of_range_indices():
    """The guard of vx_get_rows_f16, on the CPU only: no GPU test feeds an out-of-range index."""
    table = np.random.default_rng(8).standard_normal((10, 16)).astype(np.float16)
    idx = np.array([0, 9, 3, 3, -1, 10, 2 ** 31 - 1, -2 ** 31], np.int32)
    got = R.emulate_get_rows_kernel(table, idx)
    assert np.array_equal(got[:4], table[[0, 9, 3, 3]]) and not got[4:].any() and got.shape == (8, 16)
    assert np.array_equal(R.emulate_get_rows_kernel(table, idx[:4].reshape(2, 2)), table[[0, 9, 3, 3]].reshape(2, 2, 16))


def test_f16_floor_is_a_rounding_of_the_same_reference():
    """`rnd` only rounds: with the identity the two paths of the reference are the same function."""
    cfg = synth.SAM3_VIT_MINI
    w = synth.sam3_graph_tensors(synth.sam3_vision_state_dict(cfg, 1))
    x = np.random.default_rng(9).standard_normal((1, 8, 8, cfg.hidden))
    px, py = R.rope_2d_positions(16, 4)
    a = R.vision_layer(w, "det.ve.backbone.layers.0", x, 4, cfg.heads, (px, py, 1.0))
    b = R.vision_layer(w, "det.ve.backbone.layers.0", R.f16(x), 4, cfg.heads, (px, py, 1.0), R.f16)
    d = np.abs(a - b).max() / np.abs(a).max()
    assert 0 < d < 2e-2, d
    assert not math.isnan(d)

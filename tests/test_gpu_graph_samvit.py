"""-m gpu: the SAM ViT image encoder built through vision.cpp_amd/graph.py::sam_vit_encode at synth.SAM_VIT_MINI (96 x 96 image, a 6 x 6 grid; layer 0 in
windows of 4 on the map padded to 8 x 8, layer 1 global; batch 2) against transformers' SamVisionEncoder in float64 with the same weights.

The bound is the SAM3 mini vision encoder's (tests/test_gpu_graph_sam3.py): the reference runs once exact and once with every module's
output rounded to f16 (forward hooks on the leaf modules: where the per-node plan holds an f16 buffer); the distance of the two -- largest absolute error over
largest reference value -- is the pipeline's f16 floor, computed with no code under test, and the device may be at most 4 x that floor, fused and per node.
HF's activation is set to the tanh GELU, which is what GELU is in this layer (ggml_gelu)."""
import numpy as np
import pytest
import torch
from transformers import SamVisionConfig
from transformers.models.sam.modeling_sam import SamVisionEncoder

from visioncpp_amd import graph as G
from visioncpp_amd import synth, vision

pytestmark = pytest.mark.gpu

from gpu_util import api, release  # noqa: E402

CFG = synth.SAM_VIT_MINI
BATCH = 2


@pytest.fixture(scope="module")
def device():
    assert api().vx_device_count() > 0, "no HIP device visible: the product path has no CPU fallback"
    return vision.Device.init(vision.Backend.gpu)


@pytest.fixture(scope="module")
def reference():
    """(f16-rounded state dict, images [B, H, W, 3], exact output, output with f16 activations), outputs [B, h, w, C] float64: computed once, read-only"""
    sd = {k: v.astype(np.float16).astype(np.float64) for k, v in synth.sam_vit_state_dict(CFG, 1).items()}
    hf = SamVisionEncoder(SamVisionConfig(hidden_size=CFG.hidden, output_channels=CFG.out_channels, num_hidden_layers=CFG.n_layers, num_attention_heads=CFG.heads,
                                          image_size=CFG.image_size, patch_size=CFG.patch, window_size=CFG.window, global_attn_indexes=list(CFG.global_layers),
                                          mlp_dim=CFG.mlp, hidden_act="gelu_pytorch_tanh")).double().eval()
    hf.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    images = np.random.default_rng(41).standard_normal((BATCH, CFG.image_size, CFG.image_size, 3)).astype(np.float32)
    x = torch.from_numpy(images.astype(np.float64)).permute(0, 3, 1, 2)
    with torch.no_grad():
        exact = hf(x).last_hidden_state.permute(0, 2, 3, 1).numpy()
        hooks = [mod.register_forward_hook(lambda _m, _i, out: out.half().double()) for mod in hf.modules() if not list(mod.children())]
        floored = hf(x).last_hidden_state.permute(0, 2, 3, 1).numpy()
        for h in hooks:
            h.remove()
    return sd, images, exact, floored


def _rel(got, want):
    return float(np.abs(np.asarray(got, np.float64) - want).max() / np.abs(want).max())


def _graph(device, sd, fused, batch):
    g = G.Graph(device)
    g.set_fused_models(fused)
    for name, t in synth.sam_vit_graph_tensors(sd).items():
        g.add_weight(name, t)
    image = g.input((3, CFG.image_size, CFG.image_size, batch), G.F32, "image")
    params = G.SamVitParams(CFG.image_size, CFG.patch, CFG.window, CFG.n_layers, CFG.heads, CFG.global_layers)
    out = g.output(G.sam_vit_encode(G.ModelRef(g), image, params), "embedding")
    g.allocate()
    return g, image, out


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "per_node"])
def test_encoder_against_transformers(device, reference, fused):
    sd, images, exact, floored = reference
    floor = _rel(floored, exact)
    g, image, out = _graph(device, sd, fused, BATCH)
    g.set(image, images)
    g.compute()
    err = _rel(g.get(out), exact)
    print(f"sam_vit mini {'fused' if fused else 'per node'}: floor {floor:.3e} error {err:.3e} ratio {err / floor:.2f}")
    assert floor > 0 and err <= 4 * floor, (err, floor)
    release()


def test_one_launch_per_attention_node_and_no_square_buffer(device, reference):
    """Every ATTENTION_REL_POS node is ONE planned launch, and no buffer of the plan has room for a [T, T] tensor per (batch, head) of either layer -- the
    largest buffer is the mlp's hidden map."""
    g, _, _ = _graph(device, reference[0], True, BATCH)
    lines = g.describe().strip().splitlines()[:-1]
    attn = [line for line in lines if line.startswith("attention")]
    assert attn == ["attention_rel_pos B=8 heads=2 grid=4x4 hd=64", "attention_rel_pos B=2 heads=2 grid=6x6 hd=64"]
    assert not any("mask" in line or "bias" in line for line in lines)
    # nothing in front of an attention launch makes a bias: between the three slices of q | k | v and the attention there is no launch
    for i, line in enumerate(lines):
        if line.startswith("attention"):
            assert all(prev.startswith("slice") for prev in lines[i - 3:i]), lines[i - 3:i]
    release()

"""Depth-Anything-V2 Base and Large without a GPU: planning-only graphs (`Graph(None)`) of the full checkpoints at 518 x 518 lower
onto the wide-row LayerNorm and the Cin 64 / 128 head tail, the CPU oracle matches HuggingFace transformers at the Base widths
(tests/golden/depthany_base_short.npz, tests/golden/make_golden_depthany_variants.py), the converter writes a Base file byte for
byte as synth does, and the configs that existed before the head_hidden field write the same bytes as before."""
import hashlib

import numpy as np
import pytest

from oracle import oracle
from visioncpp_amd import _lib as L
from visioncpp_amd import convert
from visioncpp_amd import graph as G
from visioncpp_amd import synth

RTOL = 1e-3


def _plan(tmp_path_factory, cfg, batch=2, side=518):
    path = synth.write_gguf(tmp_path_factory.mktemp(cfg.name) / f"{cfg.name}.gguf", cfg, seed=0)
    g = G.Graph(None, G.Weights(path))
    img = g.input((3, side, side, batch), G.F32, "image")
    out = G.depthany_predict(G.ModelRef(g), img, cfg.n_layers, cfg.n_heads, feature_layers=cfg.feature_layers)
    g.allocate()
    return g, out


@pytest.mark.parametrize("cfg,launches,cin", [(synth.BASE, 128, 64), (synth.LARGE, 212, 128)], ids=["base", "large"])
def test_full_variants_plan_on_the_wide_kernels(tmp_path_factory, cfg, launches, cin):
    """Base 12 x 768 / Large 24 x 1024 at 518^2, batch 2: 7 launches per encoder layer on the generic path (no token-stationary block
    at these widths), every LayerNorm on the wide-row kernel, and the head's tail in ONE launch -- no full-resolution map."""
    g, out = _plan(tmp_path_factory, cfg)
    lines = g.describe().strip().splitlines()
    assert g.summary()["launches"] == len(lines) - 1 == launches
    text = "\n".join(lines)
    D, T = cfg.embed_dim, 2 * 1370
    assert not any("dino_block[" in l for l in lines)
    # LN1 + LN2 per layer, plus the shared final LayerNorm of the four taps
    assert text.count(f"layer_norm rows={T} C={D}") == 2 * cfg.n_layers + 4
    assert text.count(f"gemm[qkv heads-major] M={T} N={3 * D} K={D}") == cfg.n_layers
    assert text.count(f"attention B=2 heads={cfg.n_heads} T=1370") == cfg.n_layers
    assert text.count("gemm[gelu]") == cfg.n_layers and text.count("gemm[*scale][+res]") == 2 * cfg.n_layers
    first = next(i for i, l in enumerate(lines) if l.startswith("layer_norm"))
    per_layer = [l.split(" M=")[0].split(" rows=")[0] for l in lines[first:first + 7]]
    assert per_layer == ["layer_norm", "gemm[qkv heads-major]", f"attention B=2 heads={cfg.n_heads} T=1370", "gemm[*scale][+res]", "layer_norm",
                         "gemm[gelu]", "gemm[*scale][+res]"]
    tails = [l for l in lines if l.startswith("head_tail[")]
    assert len(tails) == 1 and tails[0] == lines[-2]
    assert tails[0].startswith(f"head_tail[resize 296x296 -> 518x518, conv3x3 {cin}->32, relu, conv1x1 -> 1, relu] B=2 <- head.conv2.weight")
    assert not any(l.startswith("bilinear_ac") and "-> 518x518" in l for l in lines)
    assert not any(l.startswith("conv1x1_to_1") for l in lines)
    assert out.dtype == G.F32 and out.ne == (1, 518, 518, 2)
    assert g.get_tensor(f"dino_layer_{cfg.feature_layers[-1]}").ne == (D, 1370, 2, 1)


def test_head_tail_support_covers_the_variant_widths():
    lib = L.get_lib()
    for cin in (64, 128):
        assert lib.vx_headconv_wide_supported(cin, 32, 518, 518, 296, 296) == 1
        assert lib.vx_headconv_wide_supported(cin, 32, 518, 700, 296, 400) == 1
        assert lib.vx_headconv_supported(cin, 32, 518, 518, 296, 296) == 0  # (the 32-channel kernel's answer is unchanged)
    assert lib.vx_headconv_wide_supported(32, 32, 518, 518, 296, 296) == 0
    assert lib.vx_headconv_wide_supported(96, 32, 518, 518, 296, 296) == 0
    assert lib.vx_headconv_wide_supported(64, 64, 518, 518, 296, 296) == 0
    assert lib.vx_headconv_wide_supported(128, 32, 518, 518, 400, 400) == 0  # a source patch too small for that scale
    assert lib.vx_headconv_wide_frag_bytes(64) == 2 * 18 * 64 * 16 and lib.vx_headconv_wide_frag_bytes(128) == 4 * 18 * 64 * 16


def test_head_tail_wide_pack_is_the_slice_order():
    """[slice][tap][ks][lane][8]: lane (cout = lane & 31, h = lane >> 5) holds W[cout][tap][32 slice + 16 ks + 8 h .. + 7]."""
    lib = L.get_lib()
    for cin in (64, 128):
        K = 9 * cin
        rows = np.arange(32 * K, dtype=np.uint16).reshape(32, K)  # (a bit pattern per position, not a value)
        out = np.zeros(lib.vx_headconv_wide_frag_bytes(cin) // 2, np.uint16)
        L.vx_check(lib.vx_headconv_wide_pack(rows.ctypes.data, cin, K, out.ctypes.data))
        o = out.reshape(cin // 32, 9, 2, 64, 8)
        for s, tap, ks, lane in [(0, 0, 0, 0), (1, 4, 1, 37), (cin // 32 - 1, 8, 1, 63), (0, 3, 0, 40)]:
            c0 = 32 * s + 16 * ks + 8 * (lane >> 5)
            np.testing.assert_array_equal(o[s, tap, ks, lane], rows[lane & 31, tap * cin + c0:tap * cin + c0 + 8])


def test_wide_layer_norm_refuses_beyond_1024(tmp_path):
    g = G.Graph(None)
    m = G.ModelRef(g)
    g.add_weight("ln.weight", np.ones(1032, np.float32), G.F32)
    g.add_weight("ln.bias", np.zeros(1032, np.float32), G.F32)
    x = g.input((1032, 10, 1, 1), G.F16)
    g.output(G.layer_norm(m["ln"], x, 1e-6), "y")
    with pytest.raises(L.Error, match="layer_norm: 1032 channels \\(a multiple of 8, at most 1024\\)"):
        g.allocate()


def test_oracle_matches_transformers_at_base_widths(golden_dir):
    """Every module boundary of HF's DepthAnythingForDepthEstimation at Base widths (4 layers, 112^2): the oracle is generic over
    widths and follows HF's head (conv1 128 -> 64, conv2 64 -> 32, conv3 32 -> 1)."""
    g = np.load(golden_dir / "depthany_base_short.npz")
    cfg = synth.BASE_SHORT
    sd = synth.state_dict(cfg, int(g["weights_seed"]))
    h = hashlib.sha256()
    for k, v in sd.items():
        h.update(k.encode())
        h.update(np.ascontiguousarray(v.astype(np.float16)).tobytes())
    assert h.hexdigest() == bytes(g["sd_sha256"]).decode(), "synthetic weights drifted from the fixture"
    assert sd["head.conv2.weight"].shape == (32, 64, 3, 3) and sd["head.conv3.weight"].shape == (1, 32, 1, 1)
    tensors, conv2d = synth.gguf_tensors(sd)
    om = oracle.Model(tensors, conv2d, "whcn")
    params = oracle.make_params(cfg.patch_size, cfg.embed_dim, cfg.n_layers, cfg.n_heads, cfg.image_size, 14, cfg.feature_layers, 1.0,
                                oracle.GELU_TANH_F32)
    img = synth.images(1, 112, 112, seed=int(g["image_seed"]))[0]
    pre = oracle.image_u8_to_f32(img, oracle.RGB_U8, oracle.RGB_F32, (-0.485, -0.456, -0.406, 0), (1 / 0.229, 1 / 0.224, 1 / 0.225, 1))
    names = sorted(k[:-len("_sample")] for k in g.files if k.endswith("_sample"))
    assert {"tokens", "layer_3", "reassemble_0", "neck_conv_3", "fusion_3", "head_conv1", "dino_layer_3"} <= set(names)
    depth, got = om.predict(params, pre, {n: 1 << 20 for n in names})
    for n in names:
        v = got[n].ravel()[::int(g[n + "_step"])]
        tol = 2e-4 if n.startswith(("layer_", "dino_layer_", "tokens")) else 5e-4
        np.testing.assert_allclose(v, g[n + "_sample"], rtol=RTOL, atol=tol, err_msg=n)
    np.testing.assert_allclose(depth, g["depth"], rtol=RTOL, atol=5e-4)


def test_converter_writes_the_synth_base_file(tmp_path):
    """tools/convert_depth_anything.py's converter on an HF-named state dict at Base widths: the same bytes as synth's writer."""
    sd = synth.state_dict(synth.BASE, seed=7)
    a = convert.convert_depth_anything(sd, tmp_path / "converted.gguf")
    b = synth.write_gguf(tmp_path / "synth.gguf", synth.BASE, sd=sd)
    assert hashlib.sha256(a.read_bytes()).hexdigest() == hashlib.sha256(b.read_bytes()).hexdigest()


# SHA-256 of the files the configs that predate head_hidden write (seed 0): head_hidden = 0 changes no byte
BEFORE = {"small": "93bf5ba070fd28994f6b86d0c2882b0e92392aa424585ab5e27fd8467d410860",
          "tiny": "f8070e0c8ab33dfd5f436c867eab213a42aa6ea0af9b6d4f9c4c3f94e27dcb0f",
          "mini": "e74f38e829e2957d693e515b37580c74dfdf7cf34cb421ff3f0f2e7def067a87",
          "short": "70fa28bb843ccf8545bd615eb4b6917df977664b04ca3a5fa627c98979048c21"}


@pytest.mark.parametrize("cfg", [synth.SMALL, synth.TINY, synth.MINI, synth.SHORT], ids=lambda c: c.name)
def test_existing_configs_write_identical_files(tmp_path, cfg):
    assert cfg.head_hidden == 0 and cfg.head_out == cfg.head_size
    p = synth.write_gguf(tmp_path / f"{cfg.name}.gguf", cfg, seed=0)
    assert hashlib.sha256(p.read_bytes()).hexdigest() == BEFORE[cfg.name]

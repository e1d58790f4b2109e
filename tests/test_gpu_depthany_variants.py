"""-m gpu: Depth-Anything-V2 Base (ViT-B, 768) and Large (ViT-L, 1024) on the MI355X. The two kernels these checkpoints needed -- the
wide-row LayerNorm (kernels_tinyvit.hip) and the head tail for Cin 64 / 128 (kernels_headconv.hip) -- against torch f32, then the
whole model through every public surface against the CPU oracle with the bounds tests/test_gpu_model.py holds Small to."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

from oracle import oracle
from tests import gpu_util as GU
from visioncpp_amd import _lib as L
from visioncpp_amd import convert, synth, vision

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]


def _rel(got, want):
    return float(np.abs(np.asarray(got, np.float64) - want).max() / max(float(np.abs(want).max()), 1e-30))


def _oracle(cfg, seed):
    sd = synth.state_dict(cfg, seed)
    tensors, conv2d = synth.gguf_tensors(sd)
    om = oracle.Model(tensors, conv2d, "whcn")
    params = oracle.make_params(cfg.patch_size, cfg.embed_dim, cfg.n_layers, cfg.n_heads, cfg.image_size, 14,
                                cfg.feature_layers, 1.0, oracle.GELU_GGML_F16_LUT)
    return om, params


def _pre(img):
    return oracle.image_u8_to_f32(img, oracle.RGB_U8, oracle.RGB_F32, (-0.485, -0.456, -0.406, 0), (1 / 0.229, 1 / 0.224, 1 / 0.225, 1))


@pytest.fixture(scope="module")
def device():
    d = vision.Device.init(vision.Backend.gpu)
    assert "gfx950" in d.description
    return d


@pytest.fixture(scope="module")
def base_path(tmp_path_factory):
    return synth.write_gguf(tmp_path_factory.mktemp("b") / "base.gguf", synth.BASE, seed=0)


@pytest.fixture(scope="module")
def base(device, base_path):
    return vision.Model.load(base_path, device)


# ---- kernels ----------------------------------------------------------------------------------------------------------------------

def _ln_ref(x, w, b, eps):
    x = x.astype(np.float64)
    m = x.mean(-1, keepdims=True)
    v = ((x - m) ** 2).mean(-1, keepdims=True)
    return ((x - m) / np.sqrt(v + eps) * w + b).astype(np.float32)


@pytest.mark.parametrize("C", [520, 768, 1024])
@pytest.mark.parametrize("rows,offset", [(1, 0.0), (7, 0.0), (333, 0.0), (2741, 0.0), (65, 300.0)])
def test_wide_layernorm_vs_f32(C, rows, offset):
    """C in (512, 1024]: one wave per row, two 16-byte chunks per lane, f32 two-pass statistics; ragged row counts (not a multiple of the
    block's four rows) and rows on a large common offset (where one-pass E[x^2] - E[x]^2 statistics would cancel)."""
    rng = np.random.default_rng(C + rows)
    x = (rng.standard_normal((rows, C)) * 1.5 + offset).astype(np.float16)
    w = (1 + 0.1 * rng.standard_normal(C)).astype(np.float32)
    b = (0.1 * rng.standard_normal(C)).astype(np.float32)
    eps = 1e-6
    want = _ln_ref(x.astype(np.float32), w, b, eps)
    lib = GU.api()
    xd, wd, bd = GU.dev(x), GU.dev(w), GU.dev(b)
    out = GU.empty(rows * C * 2 + 256)
    L.vx_check(lib.vx_layernorm_f16(xd.ptr, wd.ptr, bd.ptr, out.ptr, rows, C, eps, 0, 0, 0, None))
    out32 = GU.empty(rows * C * 4 + 256)
    L.vx_check(lib.vx_layernorm_f16(xd.ptr, wd.ptr, bd.ptr, out32.ptr, rows, C, eps, 0, 0, 1, None))
    GU.sync()
    got = out.to_numpy(np.float16, (rows * C + 128,))
    assert np.all(got[rows * C:] == 0), "wrote past the last row"
    np.testing.assert_allclose(got[:rows * C].reshape(rows, C).astype(np.float32), want, atol=4e-3, rtol=4e-3)
    tol = 2e-3 if offset else 2e-5  # (at offset 300 the f16 input itself carries 0.25 absolute rounding; the statistics stay exact)
    np.testing.assert_allclose(out32.to_numpy(np.float32, (rows * C + 64,))[:rows * C].reshape(rows, C), want, atol=tol, rtol=tol)
    GU.release()


@pytest.mark.parametrize("res,ws,C", [(9, 4, 768), (7, 7, 1024)])
def test_wide_layernorm_window_rows(res, ws, C):
    """The `res` / `ws` operands keep vx_layernorm_f16's meaning at the new widths: output rows in window order, padding = bias."""
    rng = np.random.default_rng(res * C)
    B = 2
    x = (rng.standard_normal((B, res, res, C)) * 2 + 0.3).astype(np.float16)
    w, b = (1 + 0.1 * rng.standard_normal(C)).astype(np.float32), (0.1 * rng.standard_normal(C)).astype(np.float32)
    nw = -(-res // ws)
    rows = B * nw * nw * ws * ws
    out = GU.empty(rows * C * 2)
    L.vx_check(GU.api().vx_layernorm_f16(GU.dev(x).ptr, GU.dev(w).ptr, GU.dev(b).ptr, out.ptr, rows, C, 1e-5, res, ws, 0, None))
    GU.sync()
    got = out.to_numpy(np.float16, (B, nw, nw, ws, ws, C)).astype(np.float32)
    xp = np.zeros((B, nw * ws, nw * ws, C), np.float32)
    xp[:, :res, :res] = x
    ref = _ln_ref(xp.reshape(-1, C), w, b, 1e-5).reshape(B, nw, ws, nw, ws, C).transpose(0, 1, 3, 2, 4, 5)
    np.testing.assert_allclose(got, ref, atol=4e-3, rtol=4e-3)
    GU.release()


def test_wide_layernorm_limits():
    x = GU.empty(64)
    assert GU.api().vx_layernorm_f16(x.ptr, x.ptr, x.ptr, x.ptr, 1, 1032, 1e-6, 0, 0, 0, None) == 0
    assert b"at most 1024" in GU.api().vx_last_error()
    GU.release()


@pytest.mark.parametrize("cin", [64, 128])
@pytest.mark.parametrize("B,hs,ws,H,W", [(2, 296, 296, 518, 518), (1, 296, 400, 518, 700), (1, 20, 37, 35, 64)])
def test_wide_head_tail_vs_torch(cin, B, hs, ws, H, W):
    """kernels_headconv.hip, Cin 64 / 128 in 32-channel K slices: resize (bilinear, align corners) + conv 3x3 Cin -> 32 + ReLU + conv 1x1
    -> 1 + ReLU + scale against torch f32 on the same f16 operands (the resized map rounded to f16, as the kernel holds it): the
    variants' 296 -> 518, the non-square extent of a 640 x 480 request (700 x 518), and a map with ragged tiles in both directions."""
    import torch
    import torch.nn.functional as F

    lib = GU.api()
    assert lib.vx_headconv_wide_supported(cin, 32, H, W, hs, ws) == 1
    rng = np.random.default_rng(cin * 7 + H + W)
    x = (rng.standard_normal((B, hs, ws, cin)) * 0.7).astype(np.float16)
    w2 = (rng.standard_normal((32, 3, 3, cin)) / np.sqrt(9 * cin)).astype(np.float16)  # OHWI rows, k = (ky, kx, c)
    b2 = (0.1 * rng.standard_normal(32)).astype(np.float32)
    w3 = (rng.standard_normal(32) / 4).astype(np.float32)
    b3, scale = 0.05, 2.5
    rows = np.ascontiguousarray(w2.reshape(32, 9 * cin))
    frag = np.empty(lib.vx_headconv_wide_frag_bytes(cin) // 2, np.float16)
    L.vx_check(lib.vx_headconv_wide_pack(rows.ctypes.data, cin, 9 * cin, frag.ctypes.data))
    out = GU.empty(B * H * W * 4 + 256)
    L.vx_check(lib.vx_headconv_wide_bil_f16(GU.dev(x).ptr, cin, GU.dev(frag).ptr, GU.dev(b2).ptr, GU.dev(w3).ptr, b3, scale, out.ptr, B, H, W, hs, ws, None))
    GU.sync()
    flat = out.to_numpy(np.float32, (B * H * W + 64,))
    assert np.all(flat[B * H * W:] == 0), "wrote past the output"
    got = flat[:B * H * W].reshape(B, H, W)
    up = F.interpolate(torch.from_numpy(x.astype(np.float32)).permute(0, 3, 1, 2), size=(H, W), mode="bilinear", align_corners=True).half().float()
    c2 = torch.relu(F.conv2d(up, torch.from_numpy(w2.astype(np.float32)).permute(0, 3, 1, 2), torch.from_numpy(b2), padding=1))
    want = (scale * torch.relu((c2 * torch.from_numpy(w3).view(1, 32, 1, 1)).sum(1) + b3)).numpy()
    assert np.isfinite(got).all()
    err = np.abs(got - want)
    assert err.max() < 6e-3 * max(1.0, float(np.abs(want).max())), (float(err.max()), float(np.abs(want).max()))
    assert err.mean() < 6e-4
    GU.release()


def test_wide_head_tail_limits():
    lib = GU.api()
    x = GU.empty(64)
    assert lib.vx_headconv_wide_bil_f16(x.ptr, 96, x.ptr, x.ptr, x.ptr, 0.0, 1.0, x.ptr, 1, 518, 518, 296, 296, None) == 0
    assert lib.vx_headconv_wide_bil_f16(x.ptr, 64, x.ptr, x.ptr, x.ptr, 0.0, 1.0, x.ptr, 1, 518, 518, 400, 400, None) == 0
    assert b"scale up to 0.58" in lib.vx_last_error()
    GU.release()


# ---- the models -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cfg,seed", [(synth.BASE_SHORT, 5), (synth.LARGE_SHORT, 6)], ids=["base_short", "large_short"])
def test_short_variants_every_module_boundary(device, tmp_path, cfg, seed):
    model = vision.Model.load(synth.write_gguf(tmp_path / f"{cfg.name}.gguf", cfg, seed=seed), device)
    info = model.info
    assert (info.embed_dim, info.n_layers, info.n_heads) == (cfg.embed_dim, cfg.n_layers, cfg.n_heads)
    assert list(info.feature_layers) == list(cfg.feature_layers)
    om, params = _oracle(cfg, seed)
    imgs = synth.images(2, 112, 112, seed=seed + 30)
    model.enable_captures(True)
    out, raw = model.compute_batch(imgs, return_raw=True)
    model.enable_captures(False)
    names = (["tokens"] + [f"layer_{i}" for i in range(4)] + [f"dino_layer_{i}" for i in range(4)] + [f"reassemble_{i}" for i in range(4)] +
             [f"neck_conv_{i}" for i in range(4)] + [f"fusion_{i}" for i in range(4)] + ["head_conv1", "depth"])
    for b in range(2):
        caps = {n: 1 << 22 for n in names}
        depth, want = om.predict(params, _pre(imgs[b]), caps)
        for n in names:
            err = _rel(model.read_capture(n)[b].ravel(), want[n])
            assert err < 2e-2, f"{n} image {b}: rel err {err}"
        assert _rel(raw[b], depth) < 2e-2
        assert np.abs(out[b] - oracle.image_normalize(depth)).mean() < 1e-3
    fused = model.compute_batch(imgs)  # without captures the head tail is one launch
    for b in range(2):
        assert np.abs(fused[b] - oracle.image_normalize(om.predict(params, _pre(imgs[b])))).mean() < 1e-3


def test_base_518_batch2_vs_oracle(base):
    om, params = _oracle(synth.BASE, 0)
    imgs = synth.images(2, 518, 518, seed=1234)
    out, raw = base.compute_batch(imgs, return_raw=True)
    assert np.isfinite(out).all() and out.min() >= 0 and out.max() <= 1 + 1e-6
    for b in range(2):
        want_norm, want_raw = om.compute(params, imgs[b])
        mae = float(np.abs(out[b] - want_norm).mean())
        print(f"base 518 image {b}: MAE {mae:.2e}, raw rel {_rel(raw[b], want_raw):.2e}")
        assert mae < 1e-3
        assert _rel(raw[b], want_raw) < 3e-2


def test_large_518_batch1_vs_oracle(device, tmp_path):
    model = vision.Model.load(synth.write_gguf(tmp_path / "large.gguf", synth.LARGE, seed=0), device)
    assert model.info.n_layers == 24 and list(model.info.feature_layers) == [4, 11, 17, 23]
    om, params = _oracle(synth.LARGE, 0)
    img = synth.images(1, 518, 518, seed=4321)
    out, raw = model.compute_batch(img, return_raw=True)
    want_norm, want_raw = om.compute(params, img[0])
    mae = float(np.abs(out[0] - want_norm).mean())
    print(f"large 518: MAE {mae:.2e}, raw rel {_rel(raw[0], want_raw):.2e}")
    assert mae < 1e-3
    assert _rel(raw[0], want_raw) < 3e-2


def test_base_head_tail_matches_the_unfused_lowering(base):
    """With captures on, the executor keeps the head's resize and convs as separate launches (bilinear_ac, conv3x3, conv1x1_to_1); without,
    the Cin 64 head tail is one launch. 518 x 518 and the 700 x 518 extent of a 640 x 480 request."""
    for imgs in (synth.images(2, 518, 518, seed=321), synth.images(1, 700, 518, seed=9)):
        a, ra = base.compute_batch(imgs, return_raw=True)
        base.enable_captures(True)
        b, rb = base.compute_batch(imgs, return_raw=True)
        base.enable_captures(False)
        assert np.isfinite(ra).all()
        assert _rel(ra, rb) < 3e-3
        assert np.abs(a - b).mean() < 1.5e-4


def test_base_batch_independence_split_and_replay(base):
    imgs = synth.images(5, 518, 518, seed=77)
    a = base.compute_batch(imgs)
    np.testing.assert_array_equal(base.compute_batch(imgs), a)
    np.testing.assert_array_equal(base.compute_batch(imgs[3:4])[0], a[3])
    np.testing.assert_array_equal(base.compute_batch(imgs[::-1].copy())[::-1], a)
    try:
        for n in (1, 2):
            base.set_split(n)
            np.testing.assert_array_equal(base.compute_batch(imgs), a, err_msg=f"split {n}")
    finally:
        base.set_split(0)
    try:
        base.set_schedule(0)  # one launch per node (no head tail, no resizing loaders): the same numbers up to the interpolation's f16 arithmetic
        assert np.abs(base.compute_batch(imgs) - a).mean() < 3e-4
        base.set_schedule(-1)
        np.testing.assert_array_equal(base.compute_batch(imgs), a)
    finally:
        base.set_schedule(-1)
    rgb = vision.DeviceBuffer.from_numpy(imgs[:2].copy())
    out = vision.DeviceBuffer(2 * 518 * 518 * 4)
    base.use_graph(True)
    try:
        for _ in range(3):
            base.compute_batch_device(rgb.ptr, 2, 518, 518, out.ptr)
            np.testing.assert_array_equal(out.to_numpy(np.float32, (2, 518, 518)), a[:2])
    finally:
        base.use_graph(False)
    base.compute_batch_device(rgb.ptr, 2, 518, 518, out.ptr)
    np.testing.assert_array_equal(out.to_numpy(np.float32, (2, 518, 518)), a[:2])


def test_base_overlapped_pipeline(base):
    imgs = synth.images(6, 518, 518, seed=91)
    want = base.compute_batch(imgs)
    base.use_graph(True)
    pipe = vision.DepthPipeline(base, 2, 518, 518, n_slots=3)
    try:
        tickets = [pipe.submit(imgs[i:i + 2]) for i in (0, 2, 4)]
        got = [pipe.wait(t) for t in tickets]
        np.testing.assert_array_equal(np.concatenate(got), want)
    finally:
        pipe.close()
        base.use_graph(False)


def test_base_model_compute_rgba_640x480(base):
    """visp_model_compute on a 640 x 480 rgba image (model extent 700 x 518, alpha-weighted scale, then alpha dropped), against the
    oracle's restatement of the reference pipeline."""
    assert base.image_extent(640, 480) == (700, 518)
    om, params = _oracle(synth.BASE, 0)
    wide = synth.images(1, 640, 480, seed=10)[0]
    rng = np.random.default_rng(3)
    alpha = (rng.random((480, 640, 1)) * 255).astype(np.uint8)
    alpha[:, :320] = 255
    rgba = np.concatenate([wide, alpha], axis=-1)
    res = base.compute(rgba, vision.ImageFormat.rgba_u8)
    assert res.shape == (480, 640) and res.dtype == np.uint8
    ew, eh = base.image_extent(640, 480)
    scaled = oracle.image_scale(rgba, oracle.RGBA_U8, ew, eh)[..., :3]
    want, _ = om.compute(params, np.ascontiguousarray(scaled))
    back = oracle.image_scale(want, oracle.ALPHA_F32, 640, 480)
    want8 = oracle.image_f32_to_u8(oracle.image_normalize(back)[..., None], oracle.ALPHA_F32, oracle.ALPHA_U8)[..., 0]
    d = np.abs(res.astype(int) - want8.astype(int))
    assert d.max() <= 3 and d.mean() < 0.5, (d.max(), d.mean())
    rgb = base.compute(wide)  # and rgb of any extent
    assert rgb.shape == (480, 640) and np.abs(rgb.astype(int) - res.astype(int)).max() > 3


def test_converted_base_checkpoint_is_identical(device, tmp_path, base):
    sd = synth.state_dict(synth.BASE, seed=0)
    conv = vision.Model.load(convert.convert_depth_anything(sd, tmp_path / "converted.gguf"), device)
    imgs = synth.images(2, 518, 518, seed=55)
    np.testing.assert_array_equal(conv.compute_batch(imgs), base.compute_batch(imgs))


def test_public_cpp_header_on_a_base_file(tmp_path):
    """include/visp/vision.h in the installed-package caller (tests/cpp/pkg_check.cpp) on a file at Base widths."""
    exe = ROOT / "vision.cpp_amd" / "lib" / "pkg_check"
    assert exe.exists(), "run __graft_entry__.build() first"
    path = synth.write_gguf(tmp_path / "base_short.gguf", synth.BASE_SHORT, seed=5)
    r = subprocess.run([str(exe), str(path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "pkg_check ok" in r.stdout, (r.stdout, r.stderr)

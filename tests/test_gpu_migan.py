"""MI-GAN inpainting on the MI355X (csrc/kernels_migan.hip, csrc/migan.cpp) against the numpy oracle tests/migan_ref.py
(itself pinned on the reference's torch modules by tests/test_oracle_migan.py): each kernel, the whole generator at 256 and
512 with the real channel table, migan_compute at other extents, batch entry, captures and the error paths."""
import ctypes as C
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tests"))
import migan_ref  # noqa: E402
from visioncpp_amd import _lib as L  # noqa: E402
from visioncpp_amd import synth, vision  # noqa: E402

pytestmark = pytest.mark.gpu

GEN_TOL = 5e-3  # generator f32 output, outputs of order 1 (measured max 1.3e-3 at 512)


@pytest.fixture(autouse=True)
def _release():
    yield
    from tests import gpu_util as G
    G.release()


@pytest.fixture(scope="module")
def device():
    return vision.Device.init(vision.Backend.gpu)


_cache: dict = {}


def _model(device, tmp_path_factory, res: int, seed: int):
    key = ("model", res, seed)
    if key not in _cache:
        sd = synth.migan_state_dict(res, seed=seed)
        path = synth.write_migan_gguf(tmp_path_factory.mktemp("migan") / f"migan{res}.gguf", res, sd=sd)
        _cache[key] = (vision.Migan.load(path, device), migan_ref.f16_rounded(sd), path)
    return _cache[key]


def _inputs(n: int, res: int, seed: int, channels: int = 3):
    rng = np.random.default_rng(seed)
    imgs = synth.images(n, res, res, seed=seed)
    if channels == 4:
        imgs = np.concatenate([imgs, rng.integers(0, 256, imgs.shape[:3] + (1,), dtype=np.uint8)], -1)
    masks = np.zeros((n, res, res), np.uint8)
    for i in range(n):
        y0, x0 = rng.integers(0, res // 2, 2)
        masks[i, y0:y0 + res // 3, x0:x0 + res // 4] = 255
        masks[i, rng.integers(0, res), :] = 128
    return imgs, masks


# ---- kernels ----------------------------------------------------------------------------------------------------

def _dw_weights(rng, C):
    w = (rng.standard_normal((C, 1, 3, 3)) / 3).astype(np.float16).astype(np.float32)
    b = (rng.standard_normal(C) * 0.1).astype(np.float32)
    return w, b


def _fir_dev(f):  # torch [C,1,4,4] -> f32 [16][C]
    from tests import gpu_util as G
    return G.dev(np.ascontiguousarray(f[:, 0].reshape(f.shape[0], 16).T).astype(np.float32))


@pytest.mark.parametrize("C_", [64, 128, 256, 512])
@pytest.mark.parametrize("down", [False, True])
def test_dwconv_kernel(C_, down):
    from tests import gpu_util as G
    rng = np.random.default_rng(C_ + down)
    B, H, W = 2, 16, 24
    x = rng.standard_normal((B, H, W, C_)).astype(np.float16)
    w, b = _dw_weights(rng, C_)
    f = synth._migan_fir(rng, C_, 1.0)
    want = migan_ref.lrelu_agc(migan_ref.depthwise(x.astype(np.float32), w, b, 1, 1))
    if down:
        want = migan_ref.downsample(want, f)
    OH, OW = want.shape[1:3]
    y = G.empty(B * OH * OW * C_ * 2)
    wdev = G.dev(np.ascontiguousarray(w[:, 0].reshape(C_, 9).T).astype(np.float16))
    L.vx_check(G.api().vx_migan_dwconv_f16(G.dev(x).ptr, wdev.ptr, G.dev(b).ptr, _fir_dev(f).ptr if down else None, y.ptr, B, H, W, C_, None))
    G.sync()
    got = y.to_numpy(np.float16, (B, OH, OW, C_)).astype(np.float32)
    np.testing.assert_allclose(got, want, atol=1e-2, rtol=1e-2)


@pytest.mark.parametrize("noise,res1", [(False, False), (True, False), (False, True), (True, True)])
def test_gemm_lrelu_agc_epilogue(noise, res1):
    from tests import gpu_util as G
    rng = np.random.default_rng(3)
    B, R, K, N = 2, 16, 128, 64
    M = B * R * R
    a = rng.standard_normal((M, K)).astype(np.float16)
    w = (rng.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32)
    bias = (rng.standard_normal(N) * 0.1).astype(np.float32)
    nz = rng.standard_normal(R * R).astype(np.float32) * 0.3
    r1 = rng.standard_normal((M, N)).astype(np.float16)
    acc = a.astype(np.float32) @ w.astype(np.float16).astype(np.float32).T + bias
    if noise:
        acc = acc + np.tile(nz, B)[:, None]
    want = migan_ref.lrelu_agc(acc)
    if res1:
        want = want + r1.astype(np.float32)
    out = G.empty(M * N * 2)
    kw = dict(n_valid=N)
    if noise:
        kw.update(noise=G.dev(nz), noise_hw=R * R)
    if res1:
        kw.update(res1=G.dev(r1))
    G.gemm(G.dev(a), G.pad_weight(w), bias, M, L.EPI_LRELU_AGC, out=out, ldo=N, **kw)
    got = out.to_numpy(np.float16, (M, N)).astype(np.float32)
    np.testing.assert_allclose(got, want, atol=2e-2, rtol=1e-2)


def test_upsample_kernel_with_noise_and_feat():
    from tests import gpu_util as G
    rng = np.random.default_rng(4)
    B, h, w, C_ = 2, 8, 4, 128
    y = rng.standard_normal((B, h, w, C_)).astype(np.float16)
    f = synth._migan_fir(rng, C_, 4.0)
    nz = rng.standard_normal((2 * h, 2 * w)).astype(np.float32) * 0.2
    feat = rng.standard_normal((B, 2 * h, 2 * w, C_)).astype(np.float16)
    want = migan_ref.lrelu_agc(migan_ref.upsample(y.astype(np.float32), f) + nz[None, :, :, None]) + feat.astype(np.float32)
    out = G.empty(B * 4 * h * w * C_ * 2)
    L.vx_check(G.api().vx_migan_upsample_f16(G.dev(y).ptr, _fir_dev(f).ptr, G.dev(nz).ptr, G.dev(feat).ptr, out.ptr, B, h, w, C_, None))
    G.sync()
    got = out.to_numpy(np.float16, (B, 2 * h, 2 * w, C_)).astype(np.float32)
    np.testing.assert_allclose(got, want, atol=1e-2, rtol=1e-2)


@pytest.mark.parametrize("with_prev", [False, True])
def test_torgb_kernel(with_prev):
    from tests import gpu_util as G
    rng = np.random.default_rng(5)
    B, H, W, C_ = 2, 16, 8, 512
    x = rng.standard_normal((B, H, W, C_)).astype(np.float16)
    wt = (rng.standard_normal((3, C_, 1, 1)) / np.sqrt(C_)).astype(np.float32)
    bias = rng.standard_normal(3).astype(np.float32)
    prev = rng.standard_normal((B, H // 2, W // 2, 3)).astype(np.float32)
    f = synth._migan_fir(rng, 3, 4.0)
    want = migan_ref.conv1x1(x.astype(np.float32), wt, bias)
    if with_prev:
        want = want + migan_ref.upsample(prev, f)
    out = G.empty(B * H * W * 3 * 4)
    L.vx_check(G.api().vx_migan_torgb(G.dev(x).ptr, G.dev(np.ascontiguousarray(wt[:, :, 0, 0])).ptr, G.dev(bias).ptr,
                                      G.dev(prev).ptr if with_prev else None, _fir_dev(f).ptr, out.ptr, B, H, W, C_, None))
    G.sync()
    np.testing.assert_allclose(out.to_numpy(np.float32, (B, H, W, 3)), want, atol=1e-3, rtol=1e-3)


# ---- whole generator ---------------------------------------------------------------------------------------------

def _oracle_gen(sd, res, x4, key):
    if key not in _cache:
        _cache[key] = migan_ref.generate(sd, x4, res)
    return _cache[key]


@pytest.mark.parametrize("res,batch", [(256, 1), (256, 4), (512, 1)])
def test_generator_against_oracle(device, tmp_path_factory, res, batch):
    model, sd, _ = _model(device, tmp_path_factory, res, seed=1)
    assert model.info == dict(resolution=res, channels=synth.migan_channels(res))
    imgs, masks = _inputs(batch, res, seed=20)
    x4 = np.stack([migan_ref.preprocess(imgs[i], masks[i], res) for i in range(batch)])
    want = np.concatenate([_oracle_gen(sd, res, x4[i:i + 1], ("gen", res, 20, i)) for i in range(batch)])
    got = model.generate(x4)
    err = float(np.abs(got - want).max())
    assert err <= GEN_TOL, (err, float(np.abs(want).max()))


def _u8_close(got, want):
    d = np.abs(got.astype(np.int32) - want.astype(np.int32))
    assert d.max() <= 2 and (d <= 1).mean() >= 0.999, (int(d.max()), float((d <= 1).mean()))


@pytest.mark.parametrize("res", [256, 512])
def test_batch_entry_against_oracle_and_single(device, tmp_path_factory, res):
    """compute_batch (device pre / post processing, hipGraph replay) = the oracle's pipeline at the model extent; batch results
    are bit-identical to single-image results."""
    model, sd, _ = _model(device, tmp_path_factory, res, seed=1)
    imgs, masks = _inputs(4, res, seed=20)
    got = model.compute_batch(imgs, masks)
    got_again = model.compute_batch(imgs, masks)  # replay of the captured graph
    np.testing.assert_array_equal(got_again, got)
    for i in range(4):
        single = model.compute_batch(imgs[i:i + 1], masks[i:i + 1])
        np.testing.assert_array_equal(single[0], got[i])
    for i in range(1 if res == 512 else 4):
        x4 = migan_ref.preprocess(imgs[i], masks[i], res)[None]
        rgb = _oracle_gen(sd, res, x4, ("gen", res, 20, i))[0]
        want = migan_ref.postprocess(rgb, masks[i])
        _u8_close(got[i], want)
        np.testing.assert_array_equal(got[i][..., 3], masks[i])


def test_graph_recaptured_after_workspace_growth(device, tmp_path_factory):
    """Batch 1 (captured, then replayed), batch 4 (the workspace grows: the batch-1 graph is dropped), batch 1 again (captured
    anew on the new workspace, then replayed): bit-identical batch-1 results. A fresh model, so the workspace starts small."""
    _, _, path = _model(device, tmp_path_factory, 256, seed=1)
    model = vision.Migan.load(path, device)
    imgs, masks = _inputs(4, 256, seed=21)
    first = model.compute_batch(imgs[:1], masks[:1])
    np.testing.assert_array_equal(model.compute_batch(imgs[:1], masks[:1]), first)
    model.compute_batch(imgs, masks)
    for _ in range(2):
        np.testing.assert_array_equal(model.compute_batch(imgs[:1], masks[:1]), first)


@pytest.mark.parametrize("w,h,channels", [(640, 480, 3), (512, 512, 4)])
def test_migan_compute_any_extent(device, tmp_path_factory, w, h, channels):
    model, sd, _ = _model(device, tmp_path_factory, 512, seed=1)
    rng = np.random.default_rng(w + channels)
    img = synth.images(1, w, h, seed=w)[0]
    if channels == 4:
        img = np.concatenate([img, rng.integers(0, 256, (h, w, 1), dtype=np.uint8)], -1)
    mask = np.zeros((h, w), np.uint8)
    mask[h // 4:h // 2, w // 3:2 * w // 3] = 255
    got = model.compute(img, mask)
    want = migan_ref.compute(sd, 512, img, mask)
    assert got.shape == (h, w, 4)
    _u8_close(got, want)
    np.testing.assert_array_equal(got[..., 3], mask)
    # the reference's C entry: visp_model_compute(h, VISP_MIGAN, {image, mask}, 2, ...)
    iv = L.ImageView(w, h, w * channels, 3 if channels == 3 else 0, img.ctypes.data)
    mv = L.ImageView(w, h, w, 4, mask.ctypes.data)
    views = (L.ImageView * 2)(iv, mv)
    out_view, out_data = L.ImageView(), C.c_void_p()
    L.check(L.get_lib().visp_model_compute(model._handle, 3, views, 2, None, 0, C.byref(out_view), C.byref(out_data)))
    np.testing.assert_array_equal(model._take_image(out_view, out_data), got)


def test_encoder_feature_captures(device, tmp_path_factory):
    model, sd, _ = _model(device, tmp_path_factory, 256, seed=1)
    imgs, masks = _inputs(1, 256, seed=20)
    x4 = migan_ref.preprocess(imgs[0], masks[0], 256)[None]
    caps = {}
    migan_ref.generate(sd, x4, 256, caps)
    model.enable_captures(True)
    try:
        model.generate(x4)
        for r in migan_ref.levels(256):
            got = model.read_capture(f"enc.feat{r}")
            want = caps[f"enc.feat{r}"]
            assert got.shape == want.shape, (r, got.shape, want.shape)
            err = float(np.abs(got - want).max() / max(1.0, np.abs(want).max()))
            assert err <= GEN_TOL, (r, err)
        np.testing.assert_allclose(model.read_capture("syn.b256.img"), caps["syn.b256.img"], atol=GEN_TOL)
    finally:
        model.enable_captures(False)
    model.enable_timing(True)
    try:
        model.compute_batch(imgs, masks)
        names = {t["name"] for t in model.read_timing()}
        assert {"preprocess", "dwconv", "dwconv_down", "conv1x1", "upsample", "torgb", "postprocess"} <= names, names
    finally:
        model.enable_timing(False)


# ---- errors ------------------------------------------------------------------------------------------------------

def test_errors(device, tmp_path_factory, tmp_path):
    model, sd, path = _model(device, tmp_path_factory, 256, seed=1)
    api = L.get_lib()
    img = np.zeros((32, 32, 3), np.uint8)
    rgb_mask = np.zeros((32, 32, 3), np.uint8)
    iv = L.ImageView(32, 32, 96, 3, img.ctypes.data)
    with pytest.raises(L.Error, match=r"migan: second input image \(mask\) must be alpha_u8 format"):
        views = (L.ImageView * 2)(iv, L.ImageView(32, 32, 96, 3, rgb_mask.ctypes.data))
        L.check(api.visp_model_compute(model._handle, 3, views, 2, None, 0, C.byref(L.ImageView()), C.byref(C.c_void_p())))
    with pytest.raises(L.Error, match="Expected 2 input images"):
        L.check(api.visp_model_compute(model._handle, 3, (L.ImageView * 1)(iv), 1, None, 0, C.byref(L.ImageView()), C.byref(C.c_void_p())))
    with pytest.raises(L.Error, match="not built in this backend"):  # visp_model_load keeps refusing the family
        h = C.c_void_p()
        L.check(api.visp_model_load(L.path_to_char_p(path), device._handle, 3, C.byref(h)))
    esr = synth.write_esrgan_gguf(tmp_path / "esrgan.gguf", synth.ESRGAN_TINY, seed=1)
    with pytest.raises(L.Error, match="Architecture expected to be 'migan', but was 'esrgan'"):
        vision.Migan.load(esr, device)
    small = synth.migan_state_dict(16, 1024, 128, seed=2)
    bad = dict(small)
    bad["synthesis.b8.conv1.upsample.filter_const"] = np.ones_like(small["synthesis.b8.conv1.upsample.filter_const"])
    with pytest.raises(L.Error, match="zero-insertion tile"):
        vision.Migan.load(synth.write_migan_gguf(tmp_path / "bad_fc.gguf", 16, sd=bad), device)
    bad = dict(small)
    bad["encoder.b8.conv2.conv2.weight"] = np.zeros((64, 128, 1, 1), np.float32)  # 128 -> 64 where the table says 128 -> 128
    with pytest.raises(L.Error, match="encoder.b8.conv2.conv2"):
        vision.Migan.load(synth.write_migan_gguf(tmp_path / "bad_w.gguf", 16, sd=bad), device)
    # the small model itself loads and runs
    m16 = vision.Migan.load(synth.write_migan_gguf(tmp_path / "ok.gguf", 16, sd=small), device)
    imgs, masks = _inputs(1, 16, seed=3)
    x4 = migan_ref.preprocess(imgs[0], masks[0], 16)[None]
    np.testing.assert_allclose(m16.generate(x4), migan_ref.generate(migan_ref.f16_rounded(small), x4, 16), atol=GEN_TOL)


# ---- C++: the reference's test-models.cpp shape (migan_load_model -> migan_compute) -----------------------------

def test_cpp_migan_load_and_compute(device, tmp_path_factory, tmp_path):
    model, sd, path = _model(device, tmp_path_factory, 512, seed=1)
    lib_dir = ROOT / "vision.cpp_amd" / "lib"
    exe = tmp_path / "migan_check"
    subprocess.run(["g++", "-std=c++20", "-O2", "-Wall", "-Wextra", "-I", str(ROOT / "include"), str(ROOT / "tests" / "cpp" / "migan_check.cpp"),
                    "-o", str(exe), "-L", str(lib_dir), "-lvisioncpp", f"-Wl,-rpath,{lib_dir}"], check=True)
    w, h = 640, 480
    img = synth.images(1, w, h, seed=8)[0]
    mask = np.zeros((h, w), np.uint8)
    mask[100:260, 200:420] = 255
    (tmp_path / "img.raw").write_bytes(img.tobytes())
    (tmp_path / "mask.raw").write_bytes(mask.tobytes())
    r = subprocess.run([str(exe), str(path), str(tmp_path / "img.raw"), str(tmp_path / "mask.raw"), str(w), str(h), str(tmp_path / "out.raw")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "migan-check ok" in r.stdout, (r.stdout, r.stderr)
    got = np.frombuffer((tmp_path / "out.raw").read_bytes(), np.uint8).reshape(h, w, 4)
    _u8_close(got, migan_ref.compute(sd, 512, img, mask))

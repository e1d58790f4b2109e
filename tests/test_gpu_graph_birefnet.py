"""-m gpu: the kernels of csrc/kernels_imgops.hip -- the f32 image resize, image_to_patches in both forms, the pixel gate, the resize and the LayerNorm that write
through a pixel stride -- against float64 numpy (tests/imgops_ref.py), through the graph and through their launchers; encode_concat written in place against
its per-node form; and the whole birefnet_predict graph (vision.cpp_amd/graph.py) against the CPU oracle with the bounds tests/test_gpu_birefnet.py holds the
hand schedule to, with fused models and per node, replayed as a hipGraph, and with the images in reverse order.

Bounds. Image resize: 16 x the error of the same formula evaluated in numpy float32 on the same inputs (the margin covers contraction into fused multiply-adds and
operation order); where that error is zero the kernel's is too. Patches: the bits of np.float16 of the reference (the op moves and rounds). Gate: 2e-3 of the
largest value, the bound of vx_bf_mul_sigmoid_f16 (tests/test_gpu_birefnet.py). Strided resize: INTERPOLATE_BOUND of tests/test_gpu_graph_deform.py, and the bits of
vx_bilinear_ac_f16. Strided LayerNorm: 4 x the f16 floor of the reference (the rule of DESIGN.md section 14; its f32 arithmetic is far below one f16 rounding).
Every test prints its figures.

Measured on MI355X (DESIGN.md section 23 has all of it): image resize 1.3e-6 / 5.9e-7 at most against 1.3e-6 / 7.1e-7 for the formula in numpy float32, 0 where that is 0;
patches bit-equal in the three forms; gate 2.6e-4 .. 3.1e-4, fused and per node alike; strided resize 1.6e-4 / 2.9e-4, exact from 1 x 1; strided LayerNorm at the f16 floor
(2.3e-4 .. 4.1e-4); the whole graph: worst capture 3.8e-3 (feature_3), p4 .. p1 at most 2.3e-3, mask max 9.3e-4 / mean 8.8e-5 in either mode."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import imgops_ref as R
from oracle import oracle
from visioncpp_amd import _lib as L
from visioncpp_amd import graph as G
from visioncpp_amd import synth, vision

pytestmark = pytest.mark.gpu

from gpu_util import api, dev, empty, rel_err, release, sync  # noqa: E402

GATE_BOUND = 2e-3         # tests/test_gpu_birefnet.py::test_mean_broadcast_mul_sigmoid
INTERPOLATE_BOUND = 4e-3  # tests/test_gpu_graph_deform.py
SENTINEL = np.float16(-77.0)


@pytest.fixture(scope="module")
def device():
    assert api().vx_device_count() > 0, "no HIP device visible: the product path has no CPU fallback"
    return vision.Device.init(vision.Backend.gpu)


@pytest.fixture(autouse=True)
def _release_buffers():
    yield
    release()


# ---- the image resize ------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("src,dst", [((12, 8), (6, 4)), ((13, 9), (5, 4)), ((1, 1), (3, 2)), ((5, 3), (1, 1))], ids=lambda c: "x".join(map(str, c)))
@pytest.mark.parametrize("Cc", [3, 4])
def test_image_resize(device, src, dst, Cc):
    B = 2
    x = np.random.default_rng(src[0] + Cc).standard_normal((B, src[1], src[0], Cc)).astype(np.float32)
    want = R.image_bilinear_ac(x, dst[1], dst[0])
    err32 = float(np.abs(R.image_bilinear_ac(x, dst[1], dst[0], np.float32) - want).max())
    g = G.Graph(device)
    xi = g.input((Cc, src[0], src[1], B), G.F32, "image")
    y = g.output(G.interpolate(G.ModelRef(g), xi, dst, G.BILINEAR_AC), "y")
    g.allocate()
    assert g.describe().startswith(f"image_bilinear_ac {src[0]}x{src[1]} -> {dst[0]}x{dst[1]} C={Cc} B={B}")
    g.set(xi, x)
    g.compute()
    got = g.get(y)
    out = empty(want.size * 4)
    L.vx_check(api().vx_image_bilinear_ac_f32(dev(x).ptr, out.ptr, B, src[1], src[0], Cc, dst[1], dst[0], None))
    sync()
    direct = out.to_numpy(np.float32, want.shape)
    err = float(np.abs(got.astype(np.float64) - want).max())
    print(f"image resize {src} -> {dst} C={Cc}: max error {err:.3g} against float64; the formula in numpy float32: {err32:.3g}")
    assert got.shape == want.shape and err <= 16 * err32, (err, err32)
    np.testing.assert_array_equal(direct, got)  # the launcher on its own: the same bits


def test_image_resize_launcher_refusals():
    x = dev(np.zeros(64, np.float32))
    assert api().vx_image_bilinear_ac_f32(x.ptr, x.ptr, 1, 2, 2, 5, 1, 1, None) == 0 and b"1..4 channels" in api().vx_last_error()
    assert api().vx_image_bilinear_ac_f32(None, x.ptr, 1, 2, 2, 3, 1, 1, None) == 0 and b"null operand" in api().vx_last_error()
    assert api().vx_image_bilinear_ac_f32(x.ptr, x.ptr, 1, 2, 2, 3, 0, 1, None) == 0 and b"empty extent" in api().vx_last_error()


# ---- image patches ---------------------------------------------------------------------------------------------------------------------------------------

# (IW, IH, w, h, C): the three shapes of the issue; then a map wider than one LDS tile (3072 channels: 8 pixels per block, a full tile and a partial one)
# and a 4-channel image
PATCH_CASES = [(24, 16, 6, 4, 3), (16, 16, 2, 2, 3), (24, 8, 6, 4, 3), (384, 32, 12, 1, 3), (24, 16, 6, 4, 4)]


@pytest.mark.parametrize("case", PATCH_CASES, ids=lambda c: "x".join(map(str, c)))
def test_image_patches_move_and_round(device, case):
    IW, IH, w, h, Cc = case
    B, CP = 2, (IW // w) * (IH // h) * Cc
    x = np.random.default_rng(IW + IH).standard_normal((B, IH, IW, Cc)).astype(np.float32)
    want = R.image_patches(x, h, w).astype(np.float16)
    g = G.Graph(device)
    xi = g.input((Cc, IW, IH, B), G.F32, "image")
    y = g.output(G.birefnet_image_to_patches(G.ModelRef(g), xi, w, h), "patches")
    g.allocate()
    g.set(xi, x)
    g.compute()
    np.testing.assert_array_equal(g.get(y), want.astype(np.float32))
    xd = dev(x)
    tile = api().vx_image_patches_tile(CP)
    assert tile == (8 if CP == 3072 else 64)
    for form in (0, 1, 2):  # chosen by shape, naive, image rows through LDS: the same bits
        out = empty(want.size * 2, zero=False)
        L.vx_check(api().vx_image_patches_f16(xd.ptr, out.ptr, B, IH, IW, Cc, h, w, form, None))
        sync()
        np.testing.assert_array_equal(out.to_numpy(np.float16, want.shape), want, err_msg=f"form {form}")
    print(f"image patches {case}: {CP} channels, {tile} pixels per LDS tile: bit-equal in every form")


def test_image_patches_launcher_refusals():
    x, y = dev(np.zeros(24 * 16 * 3, np.float32)), empty(24 * 16 * 3 * 2)
    for args, words in (((1, 16, 24, 3, 4, 5, 0), b"Grid must divide image size"), ((1, 16, 24, 3, 16, 24, 0), b"a multiple of 8"), ((1, 16, 24, 5, 4, 6, 0), b"1..4 channels"),
                        ((1, 16, 24, 3, 4, 6, 3), b"form 3")):
        assert api().vx_image_patches_f16(x.ptr, y.ptr, *args, None) == 0 and words in api().vx_last_error(), args
    assert api().vx_image_patches_f16(x.ptr, y.ptr + 2, 1, 16, 24, 3, 4, 6, 0, None) == 0 and b"16-byte aligned" in api().vx_last_error()
    assert api().vx_image_patches_tile(48) == 64 and api().vx_image_patches_tile(3072) == 8 and api().vx_image_patches_tile(768) == 32 and api().vx_image_patches_tile(32768) == 0


# ---- the gate --------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("Cc,Cg", [(8, 8), (64, 16), (72, 16)])
def test_pixel_gate(device, Cc, Cg):
    B, Hh, Ww = 2, 5, 7  # 35 pixels per image
    rng = np.random.default_rng(Cc + Cg)
    p, a = R.f16(rng.standard_normal((B, Hh, Ww, Cc))), R.f16(rng.standard_normal((B, Hh, Ww, Cg)))
    a[1] = R.f16(a[1] * 2.0 - 0.5)  # other gate rows in the second image
    w, bias = R.f16(rng.standard_normal(Cg) * 0.5), 0.25
    rows = B * Hh * Ww
    want = R.pixel_gate(p.reshape(rows, Cc), a.reshape(rows, Cg), w, bias).reshape(p.shape)
    got = {}
    for fused in (True, False):
        g = G.Graph(device)
        g.set_fused_models(fused)
        m = G.ModelRef(g)
        g.add_weight("attn.weight", w.reshape(1, 1, 1, Cg), G.F16)
        g.add_weight("attn.bias", np.array([bias]), G.F32)
        pi, ai = g.input((Cc, Ww, Hh, B), G.F16, "p"), g.input((Cg, Ww, Hh, B), G.F16, "a")
        gate = G.repeat(m, G.sigmoid(m, G.conv_2d(m["attn"], ai)), Cc, Ww, Hh, B)
        y = g.output(G.mul(m, pi, gate), "y")
        g.allocate()
        assert g.describe().startswith("pixel_gate M=70" if fused else "conv1x1_to_1 M=70"), g.describe()
        g.set(pi, p); g.set(ai, a)
        g.compute()
        got[fused] = g.get(y)
        err = rel_err(got[fused], want)
        print(f"pixel gate C={Cc} Cg={Cg} {'fused' if fused else 'per node'}: rel_err {err:.3g}")
        assert err < GATE_BOUND, (fused, err)
    assert np.abs(R.sigmoid(a[0] @ w + bias) - R.sigmoid(a[1] @ w + bias)).max() > 0.1  # (the two images' gates differ: a kernel that read image 0's would show)
    # the launcher with leading dimensions on all three maps; what lies between the rows is not touched
    ldp, lda, ldy = Cc + 8, Cg + 16, Cc + 24
    pw, aw = np.full((rows, ldp), SENTINEL), np.full((rows, lda), SENTINEL)
    pw[:, :Cc], aw[:, 8:8 + Cg] = p.reshape(rows, Cc), a.reshape(rows, Cg)
    out = dev(np.full((rows, ldy), SENTINEL))
    L.vx_check(api().vx_pixel_gate_f16(dev(pw).ptr, ldp, dev(aw).ptr + 8 * 2, lda, dev(w.astype(np.float32)).ptr, C.c_float(bias), out.ptr + 16 * 2, ldy, rows, Cc, Cg, None))
    sync()
    o = out.to_numpy(np.float16, (rows, ldy))
    np.testing.assert_array_equal(o[:, 16:16 + Cc].astype(np.float32).reshape(p.shape), got[True])  # what the fused graph computed, to the bit
    assert np.all(o[:, :16] == SENTINEL) and np.all(o[:, 16 + Cc:] == SENTINEL)
    assert api().vx_pixel_gate_f16(dev(pw).ptr, ldp, dev(aw).ptr, lda, dev(w.astype(np.float32)).ptr, C.c_float(bias), out.ptr, Cc - 8, rows, Cc, Cg, None) == 0
    assert b"leading dimensions" in api().vx_last_error()
    assert api().vx_pixel_gate_f16(dev(pw).ptr, ldp, dev(aw).ptr, lda, dev(w.astype(np.float32)).ptr, C.c_float(bias), out.ptr, ldy, rows, Cc + 4, Cg, None) == 0
    assert b"multiples of 8" in api().vx_last_error()


# ---- the resize and the LayerNorm that write a slice of a wider map ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("src,dst", [((12, 8), (5, 3)), ((3, 2), (6, 4)), ((1, 1), (6, 4))], ids=lambda c: "x".join(map(str, c)))
def test_strided_resize_writes_its_slice_only(src, dst):
    B, Cc, x_pix, y_pix = 2, 16, 24, 40
    rng = np.random.default_rng(src[0])
    wide = rng.standard_normal((B, src[1], src[0], x_pix)).astype(np.float16)  # the source: channels [8, 24) of a 24-channel map
    x = wide[..., 8:8 + Cc]
    want = R.bilinear_ac(x, dst[1], dst[0])
    out = dev(np.full((B, dst[1], dst[0], y_pix), SENTINEL))
    L.vx_check(api().vx_bilinear_ac_pix_f16(dev(wide).ptr + 8 * 2, x_pix, out.ptr + 8 * 2, y_pix, B, src[1], src[0], Cc, dst[1], dst[0], None))
    sync()
    o = out.to_numpy(np.float16, (B, dst[1], dst[0], y_pix))
    err = rel_err(o[..., 8:24], want)
    print(f"strided resize {src} -> {dst}: rel_err {err:.3g}")
    assert err < INTERPOLATE_BOUND, err
    assert np.all(o[..., :8] == SENTINEL) and np.all(o[..., 24:] == SENTINEL), "the other 24 channels are untouched"
    plain = empty(want.size * 2)
    L.vx_check(api().vx_bilinear_ac_f16(dev(np.ascontiguousarray(x)).ptr, plain.ptr, B, src[1], src[0], Cc, dst[1], dst[0], None))
    sync()
    np.testing.assert_array_equal(plain.to_numpy(np.float16, want.shape), o[..., 8:24])  # the arithmetic of vx_bilinear_ac_f16, another destination
    assert api().vx_bilinear_ac_pix_f16(out.ptr, 12, out.ptr, y_pix, B, src[1], src[0], Cc, dst[1], dst[0], None) == 0 and b"pixel strides" in api().vx_last_error()


@pytest.mark.parametrize("Cc", [8, 72, 256, 384, 1024])  # 8, 16, 32, 64 lanes per row, and 64 lanes with two chunks each
def test_strided_layer_norm(Cc):
    rows, y_pix, off = 37, Cc + 24, 16  # 37 rows: the last block is partial in every form
    rng = np.random.default_rng(Cc)
    x = R.f16(rng.standard_normal((rows, Cc)) * 2 + 0.5)
    w, b = (1 + 0.1 * rng.standard_normal(Cc)).astype(np.float32), (0.1 * rng.standard_normal(Cc)).astype(np.float32)
    want = R.layer_norm(x, w, b, 1e-5)
    out = dev(np.full((rows, y_pix), SENTINEL))
    L.vx_check(api().vx_layernorm_pix_f16(dev(x.astype(np.float16)).ptr, dev(w).ptr, dev(b).ptr, out.ptr + off * 2, y_pix, rows, Cc, C.c_float(1e-5), None))
    sync()
    o = out.to_numpy(np.float16, (rows, y_pix))
    err, floor = rel_err(o[:, off:off + Cc], want), R.f16_floor(want)
    print(f"strided layer norm C={Cc}: rel_err {err:.3g}, the f16 floor {floor:.3g}")
    assert err <= 4 * floor, (err, floor)
    assert np.all(o[:, :off] == SENTINEL) and np.all(o[:, off + Cc:] == SENTINEL)
    assert api().vx_layernorm_pix_f16(out.ptr, dev(w).ptr, dev(b).ptr, out.ptr, Cc - 8, rows, Cc, C.c_float(1e-5), None) == 0 and b"output rows" in api().vx_last_error()


# ---- encode_concat ---------------------------------------------------------------------------------------------------------------------------------------

def test_encode_concat_in_place_gives_the_per_node_bits(device):
    features = [(32, 48, 32), (64, 24, 16), (128, 12, 8), (256, 6, 4)]
    B = 2
    rng = np.random.default_rng(3)
    data = [rng.standard_normal((B, h, w, c)).astype(np.float16) for c, w, h in features] + [rng.standard_normal((B, h // 2, w // 2, c)).astype(np.float16) for c, w, h in features]
    got = {}
    for fused in (True, False):
        g = G.Graph(device)
        g.set_fused_models(fused)
        m = G.ModelRef(g)
        xs = [g.input((c, w, h, B), G.F16, f"xs{i}") for i, (c, w, h) in enumerate(features)]
        xs_low = [g.input((c, w // 2, h // 2, B), G.F16, f"xs_low{i}") for i, (c, w, h) in enumerate(features)]
        outs = [g.output(t, f"feature_{i}") for i, t in enumerate(G.birefnet_encode_concat(m, xs, xs_low))]
        g.allocate()
        n = g.summary()["launches"]
        assert n == (11 if fused else 21), g.describe()
        for t, a in zip(xs + xs_low, data):
            g.set(t, a)
        g.compute()
        got[fused] = [g.get(t) for t in outs]
    for i, (a, b) in enumerate(zip(got[True], got[False])):
        np.testing.assert_array_equal(a, b, err_msg=f"feature_{i}")
    # and the values: the first half of every feature is the map itself, the second its half-size partner resized
    c, w, h = features[1]
    np.testing.assert_array_equal(got[True][1][..., :c], data[1].astype(np.float32))
    assert rel_err(got[True][1][..., c:], R.bilinear_ac(data[5], h, w)) < INTERPOLATE_BOUND
    assert rel_err(got[True][3][..., :64], R.bilinear_ac(got[True][0], 4, 6)) < INTERPOLATE_BOUND
    print("encode_concat: 11 launches with fused models, 21 per node, equal bits")


# ---- the whole graph -------------------------------------------------------------------------------------------------------------------------------------

SIZES = {"feature_0": 32 * 48 * 64, "feature_1": 16 * 24 * 128, "feature_2": 8 * 12 * 256, "feature_3": 4 * 6 * 960, "squeeze": 4 * 6 * 512,
         "p4": 4 * 6 * 256, "p3": 8 * 12 * 128, "p2": 16 * 24 * 64, "p1": 32 * 48 * 32}
# test_birefnet_every_level's bounds (tests/test_gpu_birefnet.py:151-158)
TOL = {"feature_0": 1e-2, "feature_1": 1e-2, "feature_2": 1e-2, "feature_3": 1.5e-2, "squeeze": 2e-2, "p4": 3e-2, "p3": 3e-2, "p2": 3e-2, "p1": 3e-2}
MEAN, STD = np.array([0.485, 0.456, 0.406], np.float32), np.array([0.229, 0.224, 0.225], np.float32)
W, H = 192, 128


@pytest.fixture(scope="module")
def mini(tmp_path_factory):
    """test_birefnet_every_level's setup: SWIN_MINI at image_size 256, seed 6, two 192 x 128 images (seed 21); the oracle's captures and masks, computed once."""
    cfg = dataclasses.replace(synth.SWIN_MINI, image_size=256)
    sd = synth.birefnet_state_dict(cfg, 6)
    path = synth.write_birefnet_gguf(tmp_path_factory.mktemp("birefnet_graph_gpu") / "mini.gguf", cfg, sd=sd)
    tensors, conv_idx = synth.birefnet_gguf_tensors(sd)
    om = oracle.Model(tensors, conv_idx)
    P = oracle.swin_params(cfg.embed_dim, cfg.window_size, cfg.depths, cfg.n_heads)
    imgs = synth.images(2, W, H, seed=21)
    pre = np.stack([((img.astype(np.float32) / 255.0 - MEAN) / STD).astype(np.float32) for img in imgs])
    want = [oracle.birefnet_predict(om, P, pre[b], captures=SIZES) for b in range(2)]
    for mask, caps in want:
        mask.setflags(write=False)
        for v in caps.values():
            v.setflags(write=False)
    return cfg, path, pre, want


def _predict(device, cfg, path, fused, hip_graph=False):
    g = G.Graph(device, G.Weights(path))
    g.set_fused_models(fused)
    m = G.ModelRef(g)
    image = g.input((3, W, H, 2), G.F32, "image")
    G.birefnet_precompute(m, (W, H), cfg.window_size)
    out = G.birefnet_predict(m, image, cfg.window_size, cfg.depths, cfg.n_heads, captures=True)
    g.allocate()
    g.use_hip_graph(hip_graph)
    return g, image, out


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "per_node"])
def test_birefnet_predict_every_level(device, mini, fused):
    cfg, path, pre, want = mini
    g, image, out = _predict(device, cfg, path, fused)
    g.set(image, pre)
    g.compute()
    masks = g.get(out).reshape(2, H, W)
    for b in range(2):
        mask, caps = want[b]
        for name in SIZES:
            got = g.get(g.get_tensor(name))[b].reshape(-1)
            e, mean = rel_err(got, caps[name]), float(np.abs(got - caps[name]).mean() / np.abs(caps[name]).max())
            print(f"{'fused' if fused else 'per node'} image {b} {name}: rel_err {e:.3g} (bound {TOL[name]:g}), mean {mean:.3g} of the largest value (4e-3)")
            assert e < TOL[name], (b, name, e)
            assert mean < 4e-3, (b, name, mean)
        d = np.abs(masks[b] - mask)
        print(f"{'fused' if fused else 'per node'} image {b} mask: max {d.max():.3g} (2e-2), mean {d.mean():.3g} (2e-3); launches {g.summary()['launches']}")
        assert d.max() < 2e-2 and d.mean() < 2e-3, (b, d.max(), d.mean())


def test_birefnet_predict_replays_and_keeps_images_apart(device, mini):
    cfg, path, pre, _ = mini
    g, image, out = _predict(device, cfg, path, True, hip_graph=True)
    g.set(image, pre)
    g.compute()  # eager: sets every kernel attribute, then records
    first = g.get(out).copy()
    for _ in range(2):  # the captured hipGraph, twice
        g.compute()
        np.testing.assert_array_equal(g.get(out), first)
    g.set(image, pre[::-1].copy())  # images are independent units
    g.compute()
    np.testing.assert_array_equal(g.get(out)[::-1], first)

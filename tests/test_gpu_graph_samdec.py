"""-m gpu: the graph layer's attention without a mask (csrc/kernels_attn_cross.hip), ggml_mul_mat of two activations, sin / cos and the Fourier features
of position_embedding_random (csrc/kernels_samdec.hip), and the SAM prompt encoder and mask decoder built through vision.cpp_amd/graph.py -- against float64
numpy on f16-rounded operands (tests/cross_attn_ref.py) and against the CPU oracle's restatement of src/visp/arch/mobile-sam.cpp:210-478.

Bounds. Attention: max(4 x the f16 floor, 4e-3) of the largest output, the masked attention's rule: P is rounded to f16 before
the second product. mul_mat: 4 x the floor (f32 sums of at most 256 products, one f16 rounding). sin / cos and the Fourier features: 4 x the floor (the
argument is reduced in f32, the hardware sine is good to about 1e-6). The decoder against the oracle: the bounds of tests/test_gpu_tinyvit.py for the hand
schedule's decoder -- mean mask error < 2 % of the mean |mask|, largest error < 0.25 x max(1, max |mask|), iou within 0.02.

Measured on MI355X (DESIGN.md section 19 has every case). Attention, error / floor of the largest output, launcher and node alike: (16, 1, 1, 1, 1) 0 / 0 (equal
to v bit for bit); (32, 3, 7, 7, 2) 3.80e-4 / 3.08e-4; (16, 2, 7, 333, 2) 2.83e-4 / 2.11e-4; (16, 8, 7, 4096, 1) 4.60e-4 / 4.60e-4; (16, 2, 333, 7, 2) 3.60e-4 / 3.60e-4;
(32, 2, 50, 77, 1) 3.14e-4 / 2.87e-4; (64, 1, 33, 65, 2) 3.04e-4 / 3.04e-4; (16, 2, 7, 333, 1) with q x 6 1.45e-4 / 1.45e-4; at the split's edges 3.0e-4 .. 4.7e-4. mul_mat,
sin, cos and the Fourier features equal their floors (1.5e-4 .. 3.8e-4); embed_points 4.79e-4 (floor 4.02e-4), embed_box 4.80e-4 (floor 3.48e-4).
sam_predict_masks against the oracle: point prompt mean error 1.11e-3 = 0.136 % of mean |mask| 0.813, largest 7.16e-3 (max |mask| 4.49), iou 5.1e-4; box prompt
1.28e-3 = 0.154 % of 0.827, largest 1.14e-2 (max |mask| 5.31), iou 3.0e-4; fused and per node give the same bits."""

import ctypes

import numpy as np
import pytest

import cross_attn_ref as R
from oracle import oracle
from visioncpp_amd import _lib as L
from visioncpp_amd import graph as G
from visioncpp_amd import synth, vision

pytestmark = pytest.mark.gpu

from gpu_util import api, dev, empty, release, sync  # noqa: E402

MODES = pytest.mark.parametrize("fused", [True, False], ids=["fused", "per_node"])


@pytest.fixture(scope="module")
def device():
    assert api().vx_device_count() > 0, "no HIP device visible: the product path has no CPU fallback"
    return vision.Device.init(vision.Backend.gpu)


@pytest.fixture(autouse=True)
def _release_buffers():
    yield
    release()


# ---- vx_attention_cross_f16 ---------------------------------------------------------------------------------------------------------------------------

ALL_ATTENTION = R.ATTENTION_CASES + R.SPLIT_EDGE_CASES
_attn_cache = {}


def _attn_case(case):
    """operands and the float64 result, computed once per case and shared by the direct and the graph tests"""
    if case not in _attn_cache:
        q, k, v = R.attention_operands(case, seed=200 + ALL_ATTENTION.index(case))
        want = R.attention(q, k, v, case[0] ** -0.5)
        for a in (q, k, v, want):
            a.setflags(write=False)
        _attn_cache[case] = (q, k, v, want)
    return _attn_cache[case]


def _check_attention(got, case, label):
    q, k, v, want = _attn_case(case)
    err, floor, bound = R.rel_err(got, want), R.f16_floor(want), R.attention_bound(want)
    print(f"attention_cross {case} {label}: err {err:.3g} floor {floor:.3g} bound {bound:.3g}")
    assert err < bound, (case, label, err, bound)
    if case[2:4] == (1, 1):  # one key: the softmax is exactly 1 and the output is v, bit for bit
        np.testing.assert_array_equal(np.asarray(got, np.float16).reshape(v.shape[0], 1, -1), v.reshape(v.shape[0], 1, -1))


def _launch_attention(case, q, k, v):
    hd, H, Tq, Tk, B, _ = case
    guard = 4 * H * hd  # rows behind the last query: queries at or beyond T_q are not stored
    out = empty((B * Tq * H * hd + guard) * 2)
    need = api().vx_attention_cross_partial_bytes(B, H, Tq, Tk, hd)
    parts = api().vx_attention_cross_parts(Tq, Tk)
    assert (need > 0) == (parts > 1) and parts == (-(-Tk // 128) if Tq <= 32 and Tk >= 256 else 1)
    part = empty(need) if need else None
    L.vx_check(api().vx_attention_cross_f16(dev(q).ptr, dev(k).ptr, dev(v).ptr, out.ptr, part.ptr if part else None, need, B, H, Tq, Tk, hd, hd ** -0.5, None))
    sync()
    got = out.to_numpy(np.float16, (B * Tq * H * hd + guard,))
    assert not got[B * Tq * H * hd:].any(), "rows behind the last query were written"
    return got[:B * Tq * H * hd].reshape(B, Tq, H * hd)


@pytest.mark.parametrize("case", ALL_ATTENTION, ids=str)
def test_attention_cross_kernel_against_float64(case):
    q, k, v, _ = _attn_case(case)
    got = _launch_attention(case, q, k, v)
    _check_attention(got, case, "launcher")
    again = _launch_attention(case, q, k, v)  # no atomics, a fixed combine order: the same bits on every run
    np.testing.assert_array_equal(got.view(np.uint16), again.view(np.uint16))


def test_attention_cross_launcher_refusals():
    q = empty(4096)
    args = (q.ptr, q.ptr, q.ptr, q.ptr)
    assert api().vx_attention_cross_f16(*args, None, 0, 1, 1, 7, 7, 48, 1.0, None) == 0 and b"head_dim 48 (16, 32 and 64 are built)" in api().vx_last_error()
    assert api().vx_attention_cross_f16(*args, None, 0, 1, 1, 7, 300, 16, 1.0, None) == 0 and b"split the keys into 3 parts and need" in api().vx_last_error()
    assert api().vx_attention_cross_f16(*args, None, 0, 1, 1, 0, 7, 16, 1.0, None) == 0 and b"empty problem" in api().vx_last_error()
    assert api().vx_attention_cross_step_f16(3, *args, None, 0, 1, 1, 7, 7, 16, 1.0, None) == 0 and b"step 3" in api().vx_last_error()


def _attention_graph(device, case, fused):
    hd, H, Tq, Tk, B, _ = case
    g = G.Graph(device)
    g.set_fused_models(fused)
    q, k, v = (g.input((hd, H, T, B), G.F16, n) for n, T in (("q", Tq), ("k", Tk), ("v", Tk)))
    y = g.output(g.op(G.OP_ATTENTION_CROSS, [q, k, v], fparams=[hd ** -0.5]), "y")
    g.allocate()
    return g, (q, k, v), y


@MODES
@pytest.mark.parametrize("case", R.ATTENTION_CASES, ids=str)
def test_attention_cross_node(device, case, fused):
    hd, H, Tq, Tk, B, _ = case
    g, ins, y = _attention_graph(device, case, fused)
    lines = g.describe().strip().splitlines()[:-1]
    parts = -(-Tk // 128) if Tq <= 32 and Tk >= 256 else 1
    head = f"attention_cross B={B} heads={H} Tq={Tq} Tk={Tk} hd={hd}"
    assert lines == ([head] if parts == 1 else [f"{head} parts={parts}", f"attention_cross_combine B={B} heads={H} Tq={Tq} parts={parts} hd={hd}"])
    for t, a in zip(ins, _attn_case(case)[:3]):
        g.set(t, a)
    g.compute()
    _check_attention(g.get(y).reshape(B, Tq, H * hd), case, "fused" if fused else "per node")


# ---- vx_mul_mat_f16 ------------------------------------------------------------------------------------------------------------------------------------

_mm_cache = {}


def _mm_case(case):
    if case not in _mm_cache:
        K, M, N, B, Ba = case
        rng = np.random.default_rng(300 + R.MUL_MAT_CASES.index(case))
        a, b = rng.standard_normal((Ba, M, K)).astype(np.float16), rng.standard_normal((B, N, K)).astype(np.float16)
        _mm_cache[case] = (a, b, R.mul_mat(a, b))
    return _mm_cache[case]


def _check_mul_mat(got, case, label):
    want = _mm_case(case)[2]
    err, floor = R.rel_err(got, want), R.f16_floor(want)
    print(f"mul_mat {case} {label}: err {err:.3g} floor {floor:.3g}")
    assert err <= 4 * floor, (case, label, err, floor)


@pytest.mark.parametrize("case", R.MUL_MAT_CASES, ids=str)
def test_mul_mat_kernel_against_float64(case):
    K, M, N, B, Ba = case
    a, b, _ = _mm_case(case)
    out = empty((B * N * M + 64) * 2)
    L.vx_check(api().vx_mul_mat_f16(dev(a).ptr, dev(b).ptr, out.ptr, M, N, K, B, Ba, None))
    sync()
    got = out.to_numpy(np.float16, (B * N * M + 64,))
    assert not got[B * N * M:].any(), "elements behind the output were written"
    _check_mul_mat(got[:B * N * M].reshape(B, N, M), case, "launcher")
    for bad, msg in (((M, N, 12, B, Ba), b"K = 12"), ((M, 17, K, B, Ba), b"N = 17"), ((M, N, 264, B, Ba), b"K = 264"), ((M, N, K, 4, 3), b"batch 3 is neither 1 nor 4")):
        assert api().vx_mul_mat_f16(out.ptr, out.ptr, out.ptr, *bad, None) == 0 and msg in api().vx_last_error(), msg


@MODES
@pytest.mark.parametrize("case", R.MUL_MAT_CASES, ids=str)
def test_mul_mat_node(device, case, fused):
    K, M, N, B, Ba = case
    g = G.Graph(device)
    g.set_fused_models(fused)
    a, b = g.input((K, M, Ba), G.F16, "a"), g.input((K, N, B), G.F16, "b")
    y = g.output(G.mul_mat(G.ModelRef(g), a, b), "y")
    g.allocate()
    assert g.describe().strip().splitlines()[:-1] == [f"mul_mat M={M} N={N} K={K} B={B}"]
    g.set(a, _mm_case(case)[0])
    g.set(b, _mm_case(case)[1])
    g.compute()
    _check_mul_mat(g.get(y).reshape(B, N, M), case, "fused" if fused else "per node")


# ---- sin / cos -------------------------------------------------------------------------------------------------------------------------------------------

@MODES
def test_sin_cos_nodes(device, fused):
    x = np.random.default_rng(7).uniform(-8, 8, 1003).astype(np.float16)  # 1003: a tail against 8 per lane
    g = G.Graph(device)
    g.set_fused_models(fused)
    m = G.ModelRef(g)
    xt = g.input((1003,), G.F16, "x")
    s, c = g.output(G.sin(m, xt), "sin"), g.output(G.cos(m, xt), "cos")
    g.allocate()
    assert g.describe().strip().splitlines()[:-1] == ["sin n=1003", "cos n=1003"]
    g.set(xt, x)
    g.compute()
    for name, t, fn in (("sin", s, np.sin), ("cos", c, np.cos)):
        want = fn(x.astype(np.float64))
        err, floor = R.rel_err(g.get(t).ravel(), want), R.f16_floor(want)
        print(f"{name} node ({'fused' if fused else 'per node'}): err {err:.3g} floor {floor:.3g}")
        assert err <= 4 * floor, (name, err, floor)


def test_sincos_launcher_tail_and_refusals():
    x = np.random.default_rng(8).uniform(-8, 8, 1003).astype(np.float16)
    for mode, fn in ((0, np.sin), (1, np.cos)):
        out = empty(1016 * 2)
        L.vx_check(api().vx_sincos_f16(mode, dev(np.concatenate([x, np.ones(13, np.float16)])).ptr, out.ptr, 1003, None))
        sync()
        got = out.to_numpy(np.float16, (1016,))
        assert not got[1003:].any(), "elements behind n were written"
        want = fn(x.astype(np.float64))
        assert R.rel_err(got[:1003], want) <= 4 * R.f16_floor(want)
    out = empty(64)
    assert api().vx_sincos_f16(2, out.ptr, out.ptr, 8, None) == 0 and b"mode 2 (0 sin, 1 cos)" in api().vx_last_error()


# ---- Fourier features and the prompt encoder -----------------------------------------------------------------------------------------------------------------

MLP, SIDE = 256, 12


@pytest.fixture(scope="module")
def decoder():
    """dim 256 (the oracle fixes 8 heads: head_dim 32 and 16), mlp 256, a 12 x 12 embedding; the oracle accepts this file (checked on the CPU: it takes res and
    dim from its arguments)"""
    sd = synth.sam_decoder_state_dict(11, mlp_dim=MLP)
    tensors = synth.sam_decoder_tensors_at(sd, SIDE)
    weights = G.Weights()
    for name, t in tensors.items():
        weights.add(name, t.astype(np.float32), G.F32 if t.dtype == np.float32 else G.F16)
    embed = np.random.default_rng(5).standard_normal((SIDE, SIDE, 256)).astype(np.float16)
    return dict(sd=sd, weights=weights, oracle=oracle.Model(tensors, [], "whcn"), embed=embed, gauss=R.f16(sd["prompt_encoder.pe_layer.positional_encoding_gaussian_matrix"]))


def test_fourier_features_kernel_against_float64(decoder):
    rng = np.random.default_rng(9)
    coords = rng.uniform(-1, 1, (37, 2)).astype(np.float32)
    gauss = decoder["gauss"]  # [2, F], f16 values
    F = gauss.shape[1]
    out = empty((37 * 2 * F + 64) * 2)
    L.vx_check(api().vx_fourier_features_f32(ctypes.cast(dev(coords).ptr, ctypes.POINTER(ctypes.c_float)), ctypes.cast(dev(np.ascontiguousarray(gauss.T, np.float32)).ptr, ctypes.POINTER(ctypes.c_float)),
                                             out.ptr, 37, F, None))
    sync()
    got = out.to_numpy(np.float16, (37 * 2 * F + 64,))
    assert not got[37 * 2 * F:].any()
    want = R.fourier_features(coords, gauss)
    err, floor = R.rel_err(got[:37 * 2 * F].reshape(37, 2 * F), want), R.f16_floor(want)
    print(f"fourier_features launcher: err {err:.3g} floor {floor:.3g} (largest argument {np.abs(2 * np.pi * coords.astype(np.float64) @ gauss).max():.3g})")
    assert err <= 4 * floor, (err, floor)


POINT, BOX = [700, 300], [200, 120, 640, 900]


def _prompt_coords(prompt):
    """the f32 coordinates the reference's caller uploads: a point and its sentinel, or the two corners"""
    return oracle.sam_process_prompt(prompt, 1024, 1024).reshape(2, 2)


@MODES
@pytest.mark.parametrize("prompt", [POINT, BOX], ids=["point", "box"])
def test_prompt_embedding_against_float64_and_the_oracle(device, decoder, prompt, fused):
    is_box = len(prompt) == 4
    coords = _prompt_coords(prompt)
    g = G.Graph(device, decoder["weights"])
    g.set_fused_models(fused)
    m = G.ModelRef(g, "prompt_encoder")
    ct = g.input((2, 2, 1), G.F32, "coords")
    y = g.output((G.sam_embed_box if is_box else G.sam_embed_points)(m, ct), "sparse")
    g.allocate()
    lines = g.describe().strip().splitlines()[:-1]
    assert sum(ln.startswith("fourier_features") for ln in lines) == 1 and not any(ln.startswith(("gemm", "mul_mat", "sin", "cos")) for ln in lines)
    g.set(ct, coords)
    g.compute()
    got = g.get(y).reshape(2, 256)
    sd = decoder["sd"]
    w = lambda name: R.f16(sd[f"prompt_encoder.{name}.weight"][0])
    pe = R.fourier_features(coords, decoder["gauss"])
    want = np.stack([pe[0] + w("point_embeddings.2"), pe[1] + w("point_embeddings.3")]) if is_box else np.stack([pe[0] + w("point_embeddings.1"), w("not_a_point_embed")])
    err, floor = R.rel_err(got, want), R.f16_floor(want)
    print(f"{'embed_box' if is_box else 'embed_points'} ({'fused' if fused else 'per node'}): err {err:.3g} floor {floor:.3g}")
    assert err <= 4 * floor, (err, floor)
    ref = oracle.sam_embed_prompt(decoder["oracle"], coords.reshape(-1), is_box)
    # the oracle test's own tolerance plus one f16 rounding of the largest value
    np.testing.assert_allclose(got, ref, rtol=1e-3, atol=2e-4 + float(np.abs(ref).max()) * 2.0 ** -11)


# ---- sam_predict_masks ------------------------------------------------------------------------------------------------------------------------------------------

def _decoder_graph(device, decoder, fused, batch):
    g = G.Graph(device, decoder["weights"])
    g.set_fused_models(fused)
    m = G.ModelRef(g)
    coords = g.input((2, 2, batch), G.F32, "coords")
    embed = g.input((256, SIDE, SIDE, 1), G.F16, "embed")
    return g, m, coords, embed


def _run_decoder(device, decoder, fused, prompts):
    """prompts: all points or all boxes, one batch entry each -> masks [B, 4, 48, 48], iou [B, 4], the graph"""
    g, m, coords, embed = _decoder_graph(device, decoder, fused, len(prompts))
    sparse = (G.sam_embed_box if len(prompts[0]) == 4 else G.sam_embed_points)(m["prompt_encoder"], coords)
    masks, iou = G.sam_predict_mask(m, embed, sparse)
    g.use_hip_graph(True)
    g.allocate()
    g.set(coords, np.stack([_prompt_coords(p) for p in prompts]))
    g.set(embed, decoder["embed"])
    g.compute()
    return g.get(masks).reshape(len(prompts), 4, 4 * SIDE, 4 * SIDE), g.get(iou).reshape(len(prompts), 4), g, masks, iou


def _mask_errors(got_masks, got_iou, want_masks, want_iou, label):
    err = np.abs(got_masks - want_masks)
    scale, peak = float(np.abs(want_masks).mean()), float(np.abs(want_masks).max())
    iou_err = float(np.abs(got_iou - want_iou).max())
    print(f"sam_predict_masks {label}: mean err {err.mean():.3g} ({err.mean() / scale:.3%} of mean |mask| {scale:.3g}) max err {err.max():.3g} (max |mask| {peak:.3g}) iou err {iou_err:.3g}")
    assert err.mean() < 0.02 * scale and err.max() < 0.25 * max(1.0, peak) and iou_err < 0.02, (label, err.mean(), scale, err.max(), peak, iou_err)


@pytest.fixture(scope="module")
def decoded(device, decoder):
    """every (mode, prompt) run once at batch 1, shared by the tests below"""
    out = {}
    for fused in (True, False):
        for name, prompt in (("point", POINT), ("box", BOX)):
            masks, iou, g, mt, it = _run_decoder(device, decoder, fused, [prompt])
            g.compute()  # the second compute replays the launch list as one hipGraph
            replay = (g.get(mt).reshape(masks.shape), g.get(it).reshape(iou.shape))
            lines = g.describe().strip().splitlines()[:-1]
            out[fused, name] = dict(masks=masks, iou=iou, replay=replay, lines=lines)
    return out


@MODES
@pytest.mark.parametrize("name,prompt", [("point", POINT), ("box", BOX)])
def test_predict_masks_against_the_oracle(decoder, decoded, name, prompt, fused):
    """Measured on MI355X: see DESIGN.md section 19."""
    d = decoded[fused, name]
    assert sum(ln.startswith("attention_cross ") for ln in d["lines"]) == 7 and not any(ln.startswith("heads_major") for ln in d["lines"])
    assert sum(ln.startswith("mul_mat") for ln in d["lines"]) == 1 and sum(ln.startswith("fourier_features") for ln in d["lines"]) == 1
    sparse = oracle.sam_embed_prompt(decoder["oracle"], _prompt_coords(prompt).reshape(-1), name == "box")
    want_masks, want_iou = oracle.sam_predict_masks(decoder["oracle"], decoder["embed"].astype(np.float32), sparse)
    _mask_errors(d["masks"][0], d["iou"][0], want_masks, want_iou, f"{name} {'fused' if fused else 'per node'} against the oracle")
    # the hipGraph replay is bit-identical
    np.testing.assert_array_equal(d["replay"][0], d["masks"])
    np.testing.assert_array_equal(d["replay"][1], d["iou"])


@pytest.mark.parametrize("name", ["point", "box"])
def test_predict_masks_fused_against_per_node(decoded, name):
    a, b = decoded[True, name], decoded[False, name]
    _mask_errors(a["masks"][0], a["iou"][0], b["masks"][0], b["iou"][0], f"{name} fused against per node")


@MODES
def test_two_prompts_are_batch_entries_with_the_bits_they_get_alone(device, decoder, decoded, fused):
    other = [300, 650]
    masks, iou, g, _, _ = _run_decoder(device, decoder, fused, [POINT, other])
    assert "attention_cross B=2 heads=8 Tq=7 Tk=144 hd=16" in g.describe()
    np.testing.assert_array_equal(masks[0], decoded[fused, "point"]["masks"][0])
    np.testing.assert_array_equal(iou[0], decoded[fused, "point"]["iou"][0])
    alone_masks, alone_iou, _, _, _ = _run_decoder(device, decoder, fused, [other])
    np.testing.assert_array_equal(masks[1], alone_masks[0])
    np.testing.assert_array_equal(iou[1], alone_iou[0])


def test_weights_that_outlive_their_graph_and_device_object_free_their_images_cleanly():
    """A Weights shared by several graphs (as the decoder fixture above) may be the last of the three to go: it keeps its device alive, so that its images are
    freed on a live device and no HIP error is left behind for the next launch of the process."""
    d = vision.Device.init(vision.Backend.gpu)
    w = G.Weights()
    w.add("c", np.ones(8, np.float32))
    g = G.Graph(d, w)
    x = g.input((8,), G.F16, "x")
    g.output(G.add(G.ModelRef(g), G.sin(G.ModelRef(g), x), G.ModelRef(g).weights("c")), "y")
    g.allocate()
    del g, x, d
    del w
    out = empty(64)
    L.vx_check(api().vx_sincos_f16(0, dev(np.zeros(8, np.float16)).ptr, out.ptr, 8, None))
    sync()

"""-m gpu: the whole Depth-Anything path through the drop-in C ABI against the CPU oracle and
the committed HuggingFace fixtures. Tolerance of the north star: per-pixel MAE < 1e-3 on the
[0,1]-normalised depth (BASELINE.json); raw-tensor checks use f16-sized relative bounds."""
import ctypes as C
import time

import numpy as np
import pytest

from oracle import oracle
from visioncpp_amd import _lib as L
from visioncpp_amd import synth, vision

pytestmark = pytest.mark.gpu


def _rel(got, want):
    return float(np.abs(np.asarray(got, np.float64) - want).max() / max(float(np.abs(want).max()), 1e-30))


@pytest.fixture(scope="module")
def device():
    d = vision.Device.init(vision.Backend.gpu)
    assert d.type is vision.Backend.gpu
    assert "gfx950" in d.description
    return d


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
def mini(device, tmp_path_factory):
    path = synth.write_gguf(tmp_path_factory.mktemp("m") / "mini.gguf", synth.MINI, seed=4)
    return vision.Model.load(path, device)


@pytest.fixture(scope="module")
def small(device, tmp_path_factory):
    path = synth.write_gguf(tmp_path_factory.mktemp("s") / "small.gguf", synth.SMALL, seed=0)
    t0 = time.time()
    m = vision.Model.load(path, device)
    print(f"load: {time.time() - t0:.3f}s")
    return m


def test_model_info(mini, small):
    i = small.info
    assert (i.patch_size, i.embed_dim, i.n_layers, i.n_heads, i.image_size) == (14, 384, 12, 6, 518)
    assert list(i.feature_layers) == [2, 5, 8, 11]
    assert small.image_extent(518, 518) == (518, 518)
    assert small.image_extent(640, 480) == (700, 518)
    assert mini.info.embed_dim == 128


def test_mini_every_module_boundary(mini):
    """Named intermediates of the HIP path vs the oracle's (the reference workbench's capture idea)."""
    cfg = synth.MINI
    om, params = _oracle(cfg, 4)
    imgs = synth.images(2, 112, 112, seed=12)
    mini.enable_captures(True)
    out, raw = mini.compute_batch(imgs, return_raw=True)
    mini.enable_captures(False)
    names = (["tokens"] + [f"layer_{i}" for i in range(4)] + [f"dino_layer_{i}" for i in range(4)] +
             [f"reassemble_{i}" for i in range(4)] + [f"neck_conv_{i}" for i in range(4)] +
             [f"fusion_{i}" for i in range(4)] + ["head_conv1", "depth"])
    for b in range(2):
        caps = {n: 1 << 22 for n in names}
        depth, want = om.predict(params, _pre(imgs[b]), caps)
        for n in names:
            got = mini.read_capture(n)[b].ravel()
            err = _rel(got, want[n])
            assert err < 2e-2, f"{n} image {b}: rel err {err}"
        assert _rel(raw[b], depth) < 2e-2
        norm = oracle.image_normalize(depth)
        assert np.abs(out[b] - norm).mean() < 1e-3, "north-star bar: MAE < 1e-3 on the normalised depth"


def test_short_every_module_boundary(device, tmp_path):
    """The block-kernel schedule (embed dim 384: csrc/kernels_block16.hip, one launch per layer between two attentions)
    at every encoder boundary, as the mini test does for the GEMM schedule; two taps name the last layer."""
    cfg = synth.SHORT
    model = vision.Model.load(synth.write_gguf(tmp_path / "short.gguf", cfg, seed=8), device)
    om, params = _oracle(cfg, 8)
    imgs = synth.images(3, 112, 112, seed=21)
    model.set_schedule(0)
    plain = model.compute_batch(imgs)  # GEMM launches
    model.set_schedule(1)
    model.enable_captures(True)
    out, raw = model.compute_batch(imgs, return_raw=True)
    model.enable_captures(False)
    names = ["tokens"] + [f"layer_{i}" for i in range(3)] + [f"dino_layer_{i}" for i in range(3)] + [f"fusion_{i}" for i in range(4)] + ["depth"]
    for b in range(3):
        caps = {n: 1 << 22 for n in names}
        depth, want = om.predict(params, _pre(imgs[b]), caps)
        for n in names:
            err = _rel(model.read_capture(n)[b].ravel(), want[n])
            assert err < 2e-2, f"{n} image {b}: rel err {err}"
        assert np.abs(out[b] - oracle.image_normalize(depth)).mean() < 1e-3
    # the two schedules agree to f16 rounding of the intermediates
    assert np.abs(plain - out).mean() < 5e-4
    model.set_schedule(0)
    np.testing.assert_array_equal(model.compute_batch(imgs), plain)
    model.set_schedule(1)
    block = model.compute_batch(imgs)  # without captures the head convs resize their inputs themselves (round 3): same numbers up to the
    # interpolation's packed-f16 arithmetic (three f16 roundings per value instead of one; this 112 x 112 configuration's depth range is
    # narrow, so the min-max normalisation magnifies it: 1.6e-4 here, 3e-5 at 518 x 518) -- and the fused path meets the bar by itself
    assert np.abs(block - out).mean() < 3e-4
    for b in range(3):
        assert np.abs(block[b] - oracle.image_normalize(om.predict(params, _pre(imgs[b])))).mean() < 1e-3
    model.set_schedule(-1)  # auto = the block kernel for this shape
    np.testing.assert_array_equal(model.compute_batch(imgs), block)


def test_mini_matches_huggingface_fixture(mini, golden_dir):
    g = np.load(golden_dir / "depthany_mini.npz")
    img = synth.images(1, 112, 112, seed=int(g["image_seed"]))
    _, raw = mini.compute_batch(img, return_raw=True)
    assert _rel(raw[0], g["depth_sample"]) < 2e-2


def test_small_518_batch_vs_oracle(small, golden_dir):
    """The north-star configuration: Depth-Anything-V2-Small, 518x518."""
    cfg = synth.SMALL
    om, params = _oracle(cfg, 0)
    imgs = synth.images(3, 518, 518, seed=1234)
    out, raw = small.compute_batch(imgs, return_raw=True)
    assert np.isfinite(out).all() and out.min() >= 0 and out.max() <= 1 + 1e-6
    for b in (0, 2):
        want_norm, want_raw = om.compute(params, imgs[b])
        mae = float(np.abs(out[b] - want_norm).mean())
        print(f"image {b}: MAE(normalised) {mae:.2e}, raw rel err {_rel(raw[b], want_raw):.2e}")
        assert mae < 1e-3
        assert _rel(raw[b], want_raw) < 3e-2
    g = np.load(golden_dir / "depthany_small.npz")  # HuggingFace transformers, same weights, image seed 1234
    assert _rel(raw[0][::7, ::7], g["depth_sample"]) < 3e-2


def test_fused_bilinear_head_matches_the_unfused_path(small):
    """Round 3: the two large `interpolate` calls of the DPT tail (fusion stage 3 -> head.conv1, head.conv1 -> head.conv2;
    depth-anything.cpp:36-38, 84-85) are done by the consumer convs' halo loaders. With captures enabled the executor keeps the
    unfused form (resize kernel + conv: `fusion_3` is a capture), so one model gives both: they differ by the interpolation's
    packed-f16 arithmetic only, far inside the MAE bar."""
    imgs = synth.images(2, 518, 518, seed=321)
    fused_out, fused_raw = small.compute_batch(imgs, return_raw=True)
    small.enable_captures(True)
    plain_out, plain_raw = small.compute_batch(imgs, return_raw=True)
    small.enable_captures(False)
    assert np.isfinite(fused_raw).all()
    assert _rel(fused_raw, plain_raw) < 3e-3
    assert np.abs(fused_raw - plain_raw).mean() < 3e-4 * np.abs(plain_raw).max()
    assert np.abs(fused_out - plain_out).mean() < 1.5e-4  # (two GPU paths against each other; each is held to MAE < 1e-3 against the oracle elsewhere)
    # 640 x 480 -> 700 x 518: a non-square extent takes the same loaders (the scale is (8 p - 1) / (14 p - 1) on both axes)
    imgs = synth.images(1, 700, 518, seed=9)
    a, ra = small.compute_batch(imgs, return_raw=True)
    small.enable_captures(True)
    b, rb = small.compute_batch(imgs, return_raw=True)
    small.enable_captures(False)
    assert _rel(ra, rb) < 3e-3 and np.abs(a - b).mean() < 1.5e-4


def test_batch_independence_and_determinism(small):
    """Images are independent units: the result for an image does not depend on its
    batch position or on the batch size, and a repeated launch is bit-identical."""
    imgs = synth.images(5, 518, 518, seed=77)
    a = small.compute_batch(imgs)
    b = small.compute_batch(imgs)
    np.testing.assert_array_equal(a, b)
    single = small.compute_batch(imgs[3:4])
    np.testing.assert_array_equal(single[0], a[3])
    rev = small.compute_batch(imgs[::-1].copy())
    np.testing.assert_array_equal(rev[::-1], a)


def test_sub_batch_split_is_bit_identical(small):
    """A step's batch runs as up to four sub-batches on parallel streams; every split gives the same bits."""
    imgs = synth.images(9, 518, 518, seed=41)
    small.set_split(1)
    want = small.compute_batch(imgs)
    try:
        for n in (2, 3, 4, 0):
            small.set_split(n)
            np.testing.assert_array_equal(small.compute_batch(imgs), want, err_msg=f"split {n}")
    finally:
        small.set_split(0)


def test_graph_replay_matches_direct_launches(small):
    imgs = synth.images(2, 518, 518, seed=5)
    want = small.compute_batch(imgs)
    rgb = vision.DeviceBuffer.from_numpy(imgs)
    out = vision.DeviceBuffer(2 * 518 * 518 * 4)
    small.use_graph(True)
    try:
        for _ in range(3):
            small.compute_batch_device(rgb.ptr, 2, 518, 518, out.ptr)
            np.testing.assert_array_equal(out.to_numpy(np.float32, (2, 518, 518)), want)
    finally:
        small.use_graph(False)


def test_graph_replay_after_step_eviction(small):
    """Four extents through the captured path evict the first one's step (three stay lowered); the first extent again is
    lowered and captured anew and gives the same bits as direct launches."""
    extents = [(112, 112), (126, 112), (112, 126), (140, 112)]
    imgs = {e: synth.images(2, e[1], e[0], seed=30 + i) for i, e in enumerate(extents)}
    w0, h0 = extents[0]
    want = small.compute_batch(imgs[extents[0]])
    small.use_graph(True)
    try:
        for w, h in extents + [extents[0]]:
            rgb = vision.DeviceBuffer.from_numpy(imgs[(w, h)])
            out = vision.DeviceBuffer(2 * w * h * 4)
            small.compute_batch_device(rgb.ptr, 2, w, h, out.ptr)
            if (w, h) == (w0, h0):
                np.testing.assert_array_equal(out.to_numpy(np.float32, (2, h0, w0)), want)
    finally:
        small.use_graph(False)


def test_reference_c_api_compute(small):
    """visp_model_compute as the reference's ctypes binding calls it (vision.py:103-128): one image of
    arbitrary extent and channel order in, alpha_u8 out. 640x480 -> model extent 700x518 (non-square, so
    the position embeddings are bicubic-resized, dino.cpp:10-30)."""
    cfg = synth.SMALL
    om, params = _oracle(cfg, 0)
    img = synth.images(1, 518, 518, seed=9)[0]
    got = small.compute(img)
    assert got.shape == (518, 518) and got.dtype == np.uint8
    want_norm, _ = om.compute(params, img)
    want_u8 = oracle.image_f32_to_u8(oracle.image_normalize(want_norm)[..., None], oracle.ALPHA_F32, oracle.ALPHA_U8)[..., 0]
    assert np.abs(got.astype(int) - want_u8.astype(int)).max() <= 2
    # bgra input of the same pixels gives the same answer (channel map, image.cpp get_channel_map)
    bgra = np.concatenate([img[..., ::-1], np.full((518, 518, 1), 255, np.uint8)], axis=-1)
    np.testing.assert_array_equal(small.compute(bgra, vision.ImageFormat.bgra_u8), got)
    # non-square input whose extent is not the model's (640x480 -> 700x518): depthany_process_input's image_scale, the pos-embed
    # interpolation, and depthany_process_output's resize back -- the whole reference call against the oracle's restatement
    wide = synth.images(1, 640, 480, seed=10)[0]
    res = small.compute(wide)
    assert res.shape == (480, 640) and res.min() == 0 and res.max() >= 254  # uint8(0.99999994*255) truncates, as in the reference
    ew, eh = small.image_extent(640, 480)
    want_n, _ = om.compute(params, oracle.image_scale(wide, oracle.RGB_U8, ew, eh))       # vision.cpp:147-160
    back = oracle.image_scale(want_n, oracle.ALPHA_F32, 640, 480)                          # depthany_process_output, vision.cpp:162-166
    want_wide = oracle.image_f32_to_u8(oracle.image_normalize(back)[..., None], oracle.ALPHA_F32, oracle.ALPHA_U8)[..., 0]  # c-api.cpp:72-77
    d = np.abs(res.astype(int) - want_wide.astype(int))
    assert d.max() <= 3 and d.mean() < 0.5, (d.max(), d.mean())
    # rgba with a varying alpha channel: depthany_process_input scales the image in ITS format (stb resizes rgba alpha-weighted) and
    # only then drops alpha (image_u8_to_f32 to rgb_f32, depth-anything.cpp:130-140) -- not the other way round
    rng = np.random.default_rng(3)
    alpha = (rng.random((480, 640, 1)) * 255).astype(np.uint8)
    alpha[:, :320] = 255
    rgba = np.concatenate([wide, alpha], axis=-1)
    res_a = small.compute(rgba, vision.ImageFormat.rgba_u8)
    scaled = oracle.image_scale(rgba, oracle.RGBA_U8, ew, eh)[..., :3]
    want_a, _ = om.compute(params, np.ascontiguousarray(scaled))
    back = oracle.image_scale(want_a, oracle.ALPHA_F32, 640, 480)
    want_a8 = oracle.image_f32_to_u8(oracle.image_normalize(back)[..., None], oracle.ALPHA_F32, oracle.ALPHA_U8)[..., 0]
    d = np.abs(res_a.astype(int) - want_a8.astype(int))
    assert d.max() <= 3 and d.mean() < 0.5, (d.max(), d.mean())
    assert np.abs(res_a.astype(int) - res.astype(int)).max() > 3  # (and it is not what the opaque image gives)


def test_non_square_extent_vs_oracle(small):
    """700x518 extent directly through the batched entry: pos-embed bicubic resize vs the oracle's."""
    cfg = synth.SMALL
    om, params = _oracle(cfg, 0)
    img = synth.images(1, 700, 518, seed=21)
    out, raw = small.compute_batch(img, return_raw=True)
    want_norm, want_raw = om.compute(params, img[0])
    assert np.abs(out[0] - want_norm).mean() < 1e-3
    assert _rel(raw[0], want_raw) < 3e-2


@pytest.mark.parametrize("executors", [2, 1])
def test_overlapped_host_pipeline_is_bit_identical(small, executors, monkeypatch):
    """visp_depthany_pipeline_*: batches streamed through 3 slots (upload / compute / download overlapped on three streams,
    consecutive forwards on two executors = two workspaces / graphs / compute streams over the same weights, or on one)
    give exactly the synchronous entry point's results, in submission order, from pageable and from pinned input; a slot
    cannot be reused before its result was read."""
    monkeypatch.setenv("VISP_PIPELINE_EXECUTORS", str(executors))
    imgs = synth.images(8, 518, 518, seed=91)
    want = small.compute_batch(imgs)
    small.use_graph(True)
    pipe = vision.DepthPipeline(small, 2, 518, 518, n_slots=3)
    tickets = [pipe.submit(imgs[0:2]), pipe.submit(imgs[2:4])]
    got = [pipe.wait(tickets[0])]
    pipe.input_view()[...] = imgs[4:6]       # fill the pinned staging buffer in place
    tickets.append(pipe.submit(None))
    tickets.append(pipe.submit(imgs[6:8]))
    got += [pipe.wait(t) for t in tickets[1:]]
    np.testing.assert_array_equal(np.concatenate(got), want)
    a, b, c = pipe.submit(imgs[0:2]), pipe.submit(imgs[2:4]), pipe.submit(imgs[4:6])
    with pytest.raises(L.Error, match="still holds an unread result"):
        pipe.submit(imgs[6:8])
    for t, lo in ((a, 0), (b, 2), (c, 4)):
        np.testing.assert_array_equal(pipe.wait(t), want[lo:lo + 2])
    with pytest.raises(L.Error, match="nothing in flight"):
        pipe.wait(a)
    pipe.close()
    small.use_graph(False)


def test_pkg_check_smoke(small):
    """The reference's installed-package smoke test (scripts/pkg-check/main.cpp:22-44): a 64x64 zero image,
    output extent equals input extent and the mean is finite."""
    res = small.compute(np.zeros((64, 64, 3), np.uint8))
    assert res.shape == (64, 64) and np.isfinite(res.astype(np.float32).mean())


def test_sharded_entry_two_models_two_threads(small, device, tmp_path):
    """visp_depthany_compute_sharded: the C-level multi-GPU entry (one model per device, one host thread each, contiguous
    shards). The box has one GPU, so both models sit on device 0 -- the sharding, the threading and the per-(kernel, device)
    attribute bookkeeping are what is exercised; results equal the single-model batch bit for bit, for uneven shards too."""
    path = synth.write_gguf(tmp_path / "small2.gguf", synth.SMALL, seed=0)
    second = vision.Model.load(path, device)
    imgs = synth.images(5, 518, 518, seed=33)
    want = small.compute_batch(imgs)
    out = np.empty((5, 518, 518), np.float32)
    handles = (C.c_void_p * 2)(small._handle, second._handle)
    L.check(L.get_lib().visp_depthany_compute_sharded(handles, 2, imgs.ctypes.data, 5, 518, 518, out.ctypes.data))  # shards 3 + 2
    np.testing.assert_array_equal(out, want)
    # larger shards go through each model's overlapped host pipeline in chunks of 32 (pinned staging, three streams, hipGraph replay):
    # 90 images -> shards of 45 = one full chunk + a partial one run as a full step; same bits as the blocking entry
    base = synth.images(10, 518, 518, seed=34)
    many = np.concatenate([base] * 9)
    for k in range(1, 9):
        many[10 * k:10 * (k + 1)] += np.uint8(29 * k)  # distinct images
    out_many = np.empty((90, 518, 518), np.float32)
    L.check(L.get_lib().visp_depthany_compute_sharded(handles, 2, many.ctypes.data, 90, 518, 518, out_many.ctypes.data))
    for lo in (0, 30, 60):
        np.testing.assert_array_equal(out_many[lo:lo + 30], small.compute_batch(many[lo:lo + 30]))
    L.check(L.get_lib().visp_depthany_compute_sharded(handles, 2, imgs.ctypes.data, 5, 518, 518, out.ctypes.data))  # and small shards after it
    np.testing.assert_array_equal(out, want)
    same = (C.c_void_p * 2)(small._handle, small._handle)
    with pytest.raises(L.Error, match="passed twice"):
        L.check(L.get_lib().visp_depthany_compute_sharded(same, 2, imgs.ctypes.data, 5, 518, 518, out.ctypes.data))


def test_two_host_threads_two_models_one_device(small, device, tmp_path):
    """Models of one visp_device share its compute stream; every entry that enqueues, captures or synchronises on it holds the device's turn
    (csrc/model.h device_turn). Two host threads, each driving its own model at the same time -- the overlapped pipeline (hipGraph capture on
    first use, then replay), visp_model_compute on an image of another extent (workspace re-reserve, eager launches, the graph is dropped and
    captured again) -- give results bit-identical to the serial runs. One run, no repeats."""
    import threading

    path = synth.write_gguf(tmp_path / "small_b.gguf", synth.SMALL, seed=0)
    other = vision.Model.load(path, device)
    imgs = synth.images(6, 518, 518, seed=77)
    one = synth.images(1, 320, 240, seed=78)[0]
    want_batch = small.compute_batch(imgs)  # serial references
    want_one = small.compute(one)
    got, errors = {}, []

    def work(tag, m):
        try:
            m.use_graph(True)
            pipe = vision.DepthPipeline(m, 2, 518, 518, n_slots=3)
            res = []
            for _ in range(3):
                tickets = [pipe.submit(imgs[k:k + 2]) for k in (0, 2, 4)]
                res.append(np.concatenate([pipe.wait(t) for t in tickets]))
                res.append(m.compute(one))
            pipe.close()
            m.use_graph(False)
            got[tag] = res
        except Exception as e:  # noqa: BLE001
            errors.append((tag, repr(e)))

    threads = [threading.Thread(target=work, args=(t, m)) for t, m in (("a", small), ("b", other))]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for tag in ("a", "b"):
        for k, r in enumerate(got[tag]):
            np.testing.assert_array_equal(r, want_batch if k % 2 == 0 else want_one)


def test_public_cpp_header_pkg_check(tmp_path):
    """include/visp/vision.h (the reference-shaped C++ API over the C ABI) in an installed-package caller (tests/cpp/pkg_check.cpp: CPU backend
    refused, two image extents, [0, 1] range, repeatable bits, image_scale); built by __graft_entry__.build(), exit code 0 = all held."""
    import subprocess
    from pathlib import Path

    exe = Path(__file__).resolve().parents[1] / "vision.cpp_amd" / "lib" / "pkg_check"
    assert exe.exists(), "run __graft_entry__.build() first"
    path = synth.write_gguf(tmp_path / "mini.gguf", synth.MINI, seed=4)
    r = subprocess.run([str(exe), str(path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "pkg_check ok" in r.stdout, (r.stdout, r.stderr)
    r = subprocess.run([str(exe), str(tmp_path / "missing.gguf")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "Failed to load GGUF model" in r.stderr


def test_public_cpp_header_depthany_pipeline(tmp_path):
    """depthany_params / depthany_detect_params / depthany_image_extent / depthany_process_input / depthany_process_output of the
    public C++ header (reference include/visp/vision.h:236-252) over the C ABI's visp_depthany_get_info, visp_image_scale,
    visp_image_u8_to_f32 and visp_image_normalize: tests/cpp/pipeline_check.cpp on the north-star configuration."""
    import subprocess
    from pathlib import Path

    exe = Path(__file__).resolve().parents[1] / "vision.cpp_amd" / "lib" / "pipeline_check"
    assert exe.exists(), "run __graft_entry__.build() first"
    path = synth.write_gguf(tmp_path / "small.gguf", synth.SMALL, seed=0)
    r = subprocess.run([str(exe), str(path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "pipeline-check ok" in r.stdout, (r.stdout, r.stderr)


def test_errors(small, device, tmp_path):
    api = L.get_lib()
    with pytest.raises(L.Error, match="multiple of the patch size"):
        small.reserve(1, 500, 500)
    with pytest.raises(L.Error, match="Expected 1 input images"):
        v = (L.ImageView * 2)()
        L.check(api.visp_model_compute(small._handle, 2, v, 2, None, 0, C.byref(L.ImageView()), C.byref(C.c_void_p())))
    with pytest.raises(L.Error, match="not built in this backend"):
        h = C.c_void_p()
        L.check(api.visp_model_load(b"/x.gguf", device._handle, 3, C.byref(h)))  # migan: a family this backend does not build
    with pytest.raises(L.Error, match="Failed to load GGUF model"):
        vision.Model.load(tmp_path / "missing.gguf", device, vision.Arch.depth_anything)


def test_weight_arena_replication(device, tmp_path):
    """The N>1 load path without the collective itself: a header-only model (VISP_LOAD_NO_UPLOAD, what ranks != 0
    do) receives the packed arena of a fully loaded model by a device copy (RCCL broadcast in bench.py) and must
    then produce bit-identical results."""
    path = synth.write_gguf(tmp_path / "mini.gguf", synth.MINI, seed=4)
    full = vision.Model.load(path, device)
    empty = vision.Model.load(path, device, no_upload=True)
    imgs = synth.images(2, 112, 112, seed=3)
    with pytest.raises(L.Error, match="not uploaded"):
        empty.compute_batch(imgs)
    (src, n), (dst, n2) = full.weights_arena(), empty.weights_arena()
    assert n == n2 and n > 0
    L.vx_check(L.get_lib().vx_memcpy_d2d(dst, src, n, None))
    L.vx_check(L.get_lib().vx_stream_sync(None))
    empty.weights_ready()
    np.testing.assert_array_equal(empty.compute_batch(imgs), full.compute_batch(imgs))


def test_small_extents_and_ragged_tiles(small):
    """Edge cases the reference's own API allows: extents far from 518 (position embeddings bicubic-resized to
    8x5 and 1x1 grids, dino.cpp:10-30), maps narrower than one conv tile, a single patch (T = 2 tokens)."""
    cfg = synth.SMALL
    om, params = _oracle(cfg, 0)
    for w, h in [(112, 70), (70, 112), (14, 14), (42, 14)]:
        img = synth.images(2, w, h, seed=w + h)
        out, raw = small.compute_batch(img, return_raw=True)
        for b in range(2):
            want_norm, want_raw = om.compute(params, img[b])
            assert _rel(raw[b], want_raw) < 3e-2, (w, h, b)
            assert np.abs(out[b] - want_norm).mean() < 2e-3, (w, h, b)


def test_batch32_properties(small):
    """BASELINE.json configs[1] at full size (batch 32, 518x518): size-independent properties -- every image is
    min-max normalised on its own (min exactly 0, max ~1), the batch equals the concatenation of two half batches,
    a checksum of per-image checksums is reproducible, and spot images match the oracle."""
    imgs = synth.images(8, 518, 518, seed=4321)
    imgs = np.concatenate([imgs, imgs[::-1], imgs[2:6], imgs[:4], imgs[4:], imgs[1:5]])[:32]
    assert imgs.shape[0] == 32
    out = small.compute_batch(imgs)
    assert out.shape == (32, 518, 518) and np.isfinite(out).all()
    assert (out.reshape(32, -1).min(axis=1) == 0).all()
    assert np.abs(out.reshape(32, -1).max(axis=1) - 1).max() < 1e-6
    halves = np.concatenate([small.compute_batch(imgs[:16]), small.compute_batch(imgs[16:])])
    np.testing.assert_array_equal(halves, out)
    sums = out.reshape(32, -1).astype(np.float64).sum(axis=1)
    np.testing.assert_array_equal(sums[:8], sums[8:16][::-1])  # same pixels -> same bits wherever they sit in the batch
    again = small.compute_batch(imgs).reshape(32, -1).astype(np.float64).sum(axis=1)
    assert float(np.sum(sums * np.arange(1, 33))) == float(np.sum(again * np.arange(1, 33)))
    om, params = _oracle(synth.SMALL, 0)
    for b in (5, 31):
        want, _ = om.compute(params, imgs[b])
        assert np.abs(out[b] - want).mean() < 1e-3


def test_converted_checkpoint_gives_identical_results(device, tmp_path):
    """safetensors -> GGUF through vision.cpp_amd/convert.py (tensor order = file order, as with the reference's
    converter) loads and computes bit-identically to the state-dict-ordered file: lookups are by name, the
    conv2d_weights list by file index."""
    from safetensors.numpy import save_file

    from visioncpp_amd import convert

    sd = synth.state_dict(synth.MINI, seed=4)
    save_file(sd, str(tmp_path / "mini.safetensors"))
    a = convert.convert_depth_anything(convert.load_safetensors(tmp_path / "mini.safetensors"), tmp_path / "a.gguf", image_size=112)
    b = synth.write_gguf(tmp_path / "b.gguf", synth.MINI, sd=sd)
    imgs = synth.images(2, 112, 112, seed=8)
    ma = vision.Model.load(a, device)
    assert (ma.info.n_layers, ma.info.n_heads, list(ma.info.feature_layers)) == (4, 2, [0, 1, 2, 3])
    np.testing.assert_array_equal(ma.compute_batch(imgs), vision.Model.load(b, device).compute_batch(imgs))

"""YOLOv9t on the MI355X (csrc/kernels_yolov9t.hip, the SiLU epilogue of kernels_gemm.hip, csrc/yolov9t.cpp) against the numpy
restatement tests/yolov9t_ref.py (itself pinned on a torch statement by tests/test_oracle_yolov9t.py): each new kernel, the network
at 256 and 640 through captures and outputs, detections against the host NMS of the library's own dense outputs, batch and hipGraph
identity, detect on 1280x720 rgb / rgba, the timing / capture tables and the error paths."""
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tests"))
import yolov9t_ref as R  # noqa: E402
from visioncpp_amd import _lib as L  # noqa: E402
from visioncpp_amd import synth, vision  # noqa: E402

pytestmark = pytest.mark.gpu

SCORE_TOL = 5e-3  # scores max abs (sigmoid outputs)
BOX_TOL = 1.0     # boxes max abs, input pixels


@pytest.fixture(autouse=True)
def _release():
    yield
    from tests import gpu_util as G
    G.release()


@pytest.fixture(scope="module")
def device():
    return vision.Device.init(vision.Backend.gpu)


_cache: dict = {}


def _model(device, tmp_path_factory, seed=0):
    if seed not in _cache:
        sd = synth.yolov9t_state_dict(seed)
        path = synth.write_yolov9t_gguf(tmp_path_factory.mktemp("yolo") / f"y{seed}.gguf", sd=sd)
        _cache[seed] = (vision.Yolov9t.load(path, device), R.f16_rounded(sd), path)
    return _cache[seed]


def _f16(a):
    return np.asarray(a, np.float32).astype(np.float16)


# ---- kernels ----------------------------------------------------------------------------------------------------

def test_silu_epilogue_conv_reads_and_writes_slices_with_a_strided_residual():
    from tests import gpu_util as G

    rng = np.random.default_rng(1)
    B, H, W, pix_in, cin, cout, pix_out = 2, 13, 11, 48, 16, 16, 40
    x = _f16(rng.standard_normal((B, H, W, pix_in)))
    w = rng.standard_normal((cout, 3, 3, cin)).astype(np.float32) / 12
    bias = rng.standard_normal(cout).astype(np.float32) * 0.1
    res = _f16(rng.standard_normal((B, H, W, 24)))
    wp = G.pad_weight(w.reshape(cout, -1))
    xd, rd = G.dev(x), G.dev(res)
    out = G.dev(np.full((B, H, W, pix_out), 7.0, np.float16))
    c0, r0, o0 = 16, 8, 24  # the conv reads channels [16, 32) of x, the residual channels [8, 24) of res, writes [24, 40) of out
    wd, bd = G.dev(wp), G.dev(G.pad_vec(bias, wp.shape[0]))
    g = L.GemmArgs()
    g.A, g.W, g.bias = xd.ptr + c0 * 2, wd.ptr, bd.ptr
    g.conv_kh = g.conv_kw = 3
    g.conv_stride, g.conv_pad, g.conv_H, g.conv_W, g.conv_Cin, g.conv_OH, g.conv_OW, g.conv_pix = 1, 1, H, W, cin, H, W, pix_in
    g.M, g.N, g.K, g.n_valid = B * H * W, wp.shape[0], wp.shape[1], cout
    g.epi, g.out, g.ldo = L.EPI_SILU, out.ptr + o0 * 2, pix_out
    g.res1, g.ld_res1 = rd.ptr + r0 * 2, 24
    L.vx_check(G.api().vx_gemm_f16(C.byref(g), None))
    G.sync()
    got = out.to_numpy(np.float16, (B, H, W, pix_out)).astype(np.float32)
    from oracle import oracle
    y = oracle.conv2d_nhwc(x[..., c0:c0 + cin].astype(np.float32), w.astype(np.float16).astype(np.float32), bias, 1, 1)
    want = R.silu(y) + res[..., r0:r0 + cout].astype(np.float32)
    assert np.abs(got[..., o0:o0 + cout] - want).max() < 2e-2
    assert np.all(got[..., :o0] == 7.0)  # nothing outside the slice is touched


def test_gemm_refuses_conv_pix_in_plain_mode_and_bad_strides():
    from tests import gpu_util as G

    a = G.dev(np.zeros((64, 64), np.float16))
    out = G.empty(64 * 64 * 2)
    with pytest.raises(L.Error, match="conv_pix"):
        G.gemm(a, np.zeros((64, 64), np.float16), None, 64, L.EPI_F16, out=out, conv_pix=64)
    with pytest.raises(L.Error, match="ld_res1"):
        G.gemm(a, np.zeros((64, 64), np.float16), None, 64, L.EPI_F16, out=out, ld_res1=64, res1=a.ptr)


def test_avgpool_spp_upsample_kernels():
    from tests import gpu_util as G

    api = G.api()
    rng = np.random.default_rng(2)
    B, H, W, C, pix = 2, 9, 12, 16, 40
    x = _f16(rng.standard_normal((B, H, W, pix)))
    xd = G.dev(x)
    y = G.empty(B * (H - 1) * (W - 1) * C * 2)
    L.vx_check(api.vx_yolo_avgpool2_f16(xd.ptr + 8 * 2, pix, y.ptr, B, H, W, C, None))
    G.sync()
    want = R.avg_pool2(x[..., 8:8 + C].astype(np.float32))
    assert np.abs(y.to_numpy(np.float16, want.shape).astype(np.float32) - want).max() < 2e-3

    buf = np.zeros((B, H, W, 4 * C + 8), np.float16)
    buf[..., :C] = x[..., :C]
    bd = G.dev(buf)
    L.vx_check(api.vx_yolo_spp_f16(bd.ptr, 4 * C + 8, B, H, W, C, None))
    G.sync()
    got = bd.to_numpy(np.float16, buf.shape).astype(np.float32)
    p1 = R.max_pool5(buf[..., :C].astype(np.float32))
    p2 = R.max_pool5(p1)
    p3 = R.max_pool5(p2)
    assert np.array_equal(got[..., C:2 * C], p1) and np.array_equal(got[..., 2 * C:3 * C], p2) and np.array_equal(got[..., 3 * C:4 * C], p3)
    assert np.all(got[..., 4 * C:] == 0)

    up = G.dev(np.zeros((B, 2 * H, 2 * W, 24), np.float16))
    L.vx_check(api.vx_yolo_upsample2_f16(xd.ptr, pix, up.ptr + 8 * 2, 24, B, H, W, C, None))
    G.sync()
    got = up.to_numpy(np.float16, (B, 2 * H, 2 * W, 24))
    assert np.array_equal(got[..., 8:], R.upsample2(x[..., :C])) and np.all(got[..., :8] == 0)
    with pytest.raises(L.Error):
        L.vx_check(api.vx_yolo_spp_f16(bd.ptr, 2 * C, B, H, W, C, None))


def test_decode_dense_and_candidates_agree():
    from tests import gpu_util as G

    api = G.api()
    rng = np.random.default_rng(3)
    B, S, nc = 2, 128, 16
    raws = [_f16(rng.standard_normal((B, S // s, S // s, 64 + nc)) * 2 - np.r_[np.zeros(64), np.full(nc, 1.5)]) for s in (8, 16, 32)]
    A = sum((S // s) ** 2 for s in (8, 16, 32))
    rd = [G.dev(r) for r in raws]
    boxes, scores = G.empty(B * A * 16), G.empty(B * A * nc * 4)
    cnt, idx, sc = G.empty(B * 4), G.empty(B * A * nc * 4), G.empty(B * A * nc * 4)
    L.vx_check(api.vx_yolo_decode(rd[0].ptr, rd[1].ptr, rd[2].ptr, B, S, nc, boxes.ptr, scores.ptr, C.c_float(0.25), cnt.ptr, idx.ptr, sc.ptr, None))
    G.sync()
    gb, gs = boxes.to_numpy(np.float32, (B, A, 4)), scores.to_numpy(np.float32, (B, A, nc))
    wb, ws = R.decode([r.astype(np.float32) for r in raws])
    assert np.abs(gb - wb).max() < 1e-3 * S and np.abs(gs - ws).max() < 1e-5
    counts = cnt.to_numpy(np.int32, (B,))
    ci, cs = idx.to_numpy(np.int32, (B, A * nc)), sc.to_numpy(np.float32, (B, A * nc))
    for b in range(B):
        n = counts[b]
        want = np.flatnonzero(gs[b].ravel() >= np.float32(0.25))
        assert n == want.size and n > 100
        order = np.argsort(ci[b, :n])
        assert np.array_equal(ci[b, :n][order], want) and np.array_equal(cs[b, :n][order], gs[b].ravel()[want])


# ---- the network --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("S", [256, 640])
def test_network_matches_the_oracle(device, tmp_path_factory, S):
    model, W, _ = _model(device, tmp_path_factory)
    x = (synth.images(1, S, S, seed=S).astype(np.float32) / 255.0)
    model.enable_captures(True)
    try:
        boxes, scores = model.forward(x)
        caps = {k: model.read_capture(f"model.{k}") for k in (2, 4, 9, 15, 21)}
        raw0 = model.read_capture("detect.raw0")
    finally:
        model.enable_captures(False)
    wb, ws, feats, raws = R.forward(W, x, return_features=True)
    errs = {}
    for k, v in caps.items():
        want = feats[k]
        assert v.shape == want.shape, (k, v.shape, want.shape)
        errs[k] = float(np.abs(v - want).max() / max(np.abs(want).max(), 1e-6))
        assert errs[k] < 2e-2, (k, errs)
    assert raw0.shape == raws[0].shape and np.abs(raw0 - raws[0]).max() < 5e-2
    e_s, e_b = float(np.abs(scores - ws).max()), float(np.abs(boxes - wb).max())
    print(f"S={S}: scores max abs {e_s:.2e}, boxes max abs {e_b:.3f} px, feature rel {errs}")
    assert e_s <= SCORE_TOL and e_b <= BOX_TOL


def test_detections_equal_host_nms_of_the_dense_outputs(device, tmp_path_factory):
    model, _, _ = _model(device, tmp_path_factory)
    imgs = synth.images(2, 256, 256, seed=21)
    boxes, scores = model.forward(imgs.astype(np.float32) / np.float32(255.0))
    got = model.detect_batch(imgs)
    for b in range(2):
        want = vision.yolov9t_nms(boxes[b], scores[b])
        assert len(want) > 0 and np.array_equal(got[b], want)
    got2 = model.detect_batch(imgs, conf=0.4, iou=0.3, max_det=20)
    for b in range(2):
        assert np.array_equal(got2[b], vision.yolov9t_nms(boxes[b], scores[b], conf=0.4, iou=0.3, max_det=20))


def test_batch_equals_single_calls_and_graph_replay(device, tmp_path_factory):
    model, _, _ = _model(device, tmp_path_factory)
    imgs = synth.images(3, 320, 320, seed=5)
    rgba = np.concatenate([imgs, np.full(imgs.shape[:3] + (1,), 17, np.uint8)], -1)
    first = model.detect_batch(imgs)
    again = model.detect_batch(imgs)  # replayed hipGraph
    singles = [model.detect_batch(imgs[i:i + 1])[0] for i in range(3)]
    four = model.detect_batch(rgba)
    for b in range(3):
        assert len(first[b]) > 0
        assert np.array_equal(first[b], again[b]) and np.array_equal(first[b], singles[b]) and np.array_equal(first[b], four[b])


def test_graph_recaptured_after_workspace_growth(device, tmp_path_factory):
    """Batch 1 (captured, then replayed), batch 4 (the workspace grows: the batch-1 graph is dropped), batch 1 again (captured
    anew on the new workspace, then replayed): equal detections. A fresh model, so the workspace starts small."""
    _, _, path = _model(device, tmp_path_factory)
    model = vision.Yolov9t.load(path, device)
    imgs = synth.images(4, 320, 320, seed=5)
    first = model.detect_batch(imgs[:1])[0]
    assert len(first) > 0
    assert np.array_equal(model.detect_batch(imgs[:1])[0], first)
    model.detect_batch(imgs)
    for _ in range(2):
        assert np.array_equal(model.detect_batch(imgs[:1])[0], first)


def _as_tuples(d):
    return [(r["x1"], r["y1"], r["x2"], r["y2"], r["confidence"], int(r["class_id"])) for r in d]


def _iou(a, b):
    iw = max(0.0, min(a[2], b[2]) - max(a[0], b[0]))
    ih = max(0.0, min(a[3], b[3]) - max(a[1], b[1]))
    union = (a[2] - a[0]) * (a[3] - a[1]) + (b[2] - b[0]) * (b[3] - b[1]) - iw * ih
    return iw * ih / union if union > 0 else 0.0


def _same_box(a, b):
    """IoU > 0.98; boxes that scale_boxes clamped to zero area (no IoU) must agree to 1 px instead."""
    iw = max(0.0, min(a[2], b[2]) - max(a[0], b[0]))
    ih = max(0.0, min(a[3], b[3]) - max(a[1], b[1]))
    inter = iw * ih
    union = (a[2] - a[0]) * (a[3] - a[1]) + (b[2] - b[0]) * (b[3] - b[1]) - inter
    if union <= 0:
        return max(abs(float(a[i]) - float(b[i])) for i in range(4)) <= 1.0
    return inter / union > 0.98


@pytest.mark.parametrize("channels", [3, 4])
def test_detect_matches_the_oracle_pipeline(device, tmp_path_factory, channels):
    model, W, _ = _model(device, tmp_path_factory)
    img = synth.images(1, 1280, 720, seed=77)[0]
    if channels == 4:
        img = np.concatenate([img, np.random.default_rng(1).integers(0, 256, img.shape[:2] + (1,), dtype=np.uint8)], -1)
    h, w = img.shape[:2]
    lb, gain, pw, ph = vision.yolov9t_letterbox(img, 640)
    rlb, rgain, rpw, rph = R.letterbox(img, 640)
    assert np.array_equal(lb, rlb) and (gain, pw, ph) == (np.float32(rgain), np.float32(rpw), np.float32(rph))
    # detect = the batch entry on the letterboxed image + scale_boxes, and the library's scale_boxes (clamp included) is the oracle's
    g_lb = model.detect_batch(lb[None])[0]
    got = model.detect(img)
    assert np.array_equal(got, vision.yolov9t_scale_boxes(g_lb, w, h, gain, pw, ph))
    want_scaled = R.scale_boxes(_as_tuples(g_lb), w, h, gain, pw, ph)
    assert [tuple(np.float32(v) for v in t[:4]) for t in want_scaled] == [(d["x1"], d["y1"], d["x2"], d["y2"]) for d in got]
    assert any(d["x1"] == 0 or d["y2"] == h for d in got)  # some boxes are clamped
    # the network + NMS against the oracle, in letterbox pixels
    wb, ws = R.forward(W, (rlb.astype(np.float32) / np.float32(255))[None])
    wb, ws = wb[0], ws[0]
    want = R.nms(wb, ws)
    assert len(want) > 5
    margin, iou_t = 0.02, 0.45
    gl = _as_tuples(g_lb)

    def ambiguous(d):
        """a same-class candidate whose score is within the margin of d's and that overlaps d, or one that is not lower by more than
        the margin and whose overlap with d is within 0.1 of the IoU threshold: the greedy order or the suppression may flip"""
        c = d[5]
        k = np.flatnonzero(ws[:, c] >= 0.25 - margin)
        ious = np.array([_iou(wb[i], d) for i in k])
        ds = ws[k, c] - d[4]
        near_order = (np.abs(ds) <= margin) & (ious > iou_t - 0.1) & (ious < 0.98)
        near_iou = (ds >= -margin) & (np.abs(ious - iou_t) < 0.1)
        return bool(np.any(near_order | near_iou))

    compared = skipped = 0
    for ref, other in ((want, gl), (gl, want)):
        for d in ref:
            if d[4] < 0.25 + margin:
                continue
            compared += 1
            if any(o[5] == d[5] and _same_box(o, d) for o in other):
                continue
            assert ambiguous(d), d
            skipped += 1
    print(f"detect {channels} channels: {compared} compared, {skipped} unmatched next to a near-tied decision")
    # measured on the MI355X: 325 compared, 97 skipped for rgb. The synthetic weights give smooth score maps, so
    # neighbouring anchors often score within the margin of each other; every skipped detection has such a competitor (asserted above)
    assert compared - skipped >= 150 and skipped <= 0.35 * compared


def test_timing_and_capture_tables(device, tmp_path_factory):
    model, _, _ = _model(device, tmp_path_factory)
    imgs = synth.images(2, 256, 256, seed=3)
    model.enable_timing(True)
    try:
        model.detect_batch(imgs)
        rows = model.read_timing()
    finally:
        model.enable_timing(False)
    names = [r["name"] for r in rows]
    assert names == ["preprocess", "conv3x3", "conv1x1", "aconv", "spp", "upsample", "head", "decode"]
    assert all(r["launches"] > 0 and r["ms"] >= 0 and r["bytes"] > 0 for r in rows)
    convs = sum(r["launches"] for r in rows if r["name"] in ("conv3x3", "conv1x1", "head")) + 5  # + the AConv stride-2 convs
    assert convs == len([c for c in synth.yolov9t_convs() if not c[0].endswith(".conv2")]), convs  # RepConv 1x1 branches are folded
    gflop = sum(r["flops"] for r in rows) / 2 / 1e9 * (640 / 256) ** 2
    assert 6.0 < gflop < 10.0, gflop  # about 8.2 GFLOP per image at 640
    model.enable_captures(True)
    try:
        model.detect_batch(imgs)
        for i in range(22):
            c = model.read_capture(f"model.{i}")
            assert c.ndim == 4 and c.shape[0] == 2
        assert model.read_capture("detect.raw2").shape == (2, 8, 8, 144)
        assert model.read_capture("scores").shape == (2, 1344, 80) and model.read_capture("boxes").shape == (2, 1344, 4)
        with pytest.raises(L.Error, match="not available"):
            model.read_capture("model.22")
    finally:
        model.enable_captures(False)
    assert model.info == dict(input_size=640, num_classes=80, reg_max=16, n_anchors=8400)


def test_error_paths(device, tmp_path_factory, tmp_path):
    model, _, _ = _model(device, tmp_path_factory)
    img = synth.images(1, 100, 100, seed=1)
    with pytest.raises(L.Error, match="multiple of 32"):
        model.detect_batch(img)
    with pytest.raises(L.Error, match="Invalid Confidence threshold"):
        model.detect(img[0], conf=2.0)
    esr = synth.write_esrgan_gguf(tmp_path / "e.gguf", synth.ESRGAN_TINY, seed=1)
    with pytest.raises(L.Error, match="Architecture expected to be 'yolov9t'"):
        vision.Yolov9t.load(esr, device)
    sd = synth.yolov9t_state_dict(1)
    del sd["model.6.cv3.0.m.1.cv1.conv2.conv.weight"]
    with pytest.raises(L.Error, match="model.6.cv3.0.m.1.cv1.conv2.conv.weight"):
        vision.Yolov9t.load(synth.write_yolov9t_gguf(tmp_path / "miss.gguf", sd=sd), device)
    sd = synth.yolov9t_state_dict(1)
    sd["model.8.cv1.conv.weight"] = sd["model.8.cv1.conv.weight"][:, :64]
    with pytest.raises(L.Error, match="model.8.cv1.conv.weight"):
        vision.Yolov9t.load(synth.write_yolov9t_gguf(tmp_path / "shape.gguf", sd=sd), device)
    sd = synth.yolov9t_state_dict(1)
    sd["detect.cv2.0.2.weight"] = sd["detect.cv2.0.2.weight"][:32]
    sd["detect.cv2.0.2.bias"] = sd["detect.cv2.0.2.bias"][:32]
    with pytest.raises(L.Error, match="reg_max 8"):
        vision.Yolov9t.load(synth.write_yolov9t_gguf(tmp_path / "reg.gguf", sd=sd), device)


def test_loader_refuses_a_class_branch_that_is_not_a_multiple_of_8(device, tmp_path):
    sd = synth.yolov9t_state_dict(2, nc=104)  # head width max(64, min(104, 100)) = 100
    with pytest.raises(L.Error, match="multiple of 8"):
        vision.Yolov9t.load(synth.write_yolov9t_gguf(tmp_path / "nc104.gguf", sd=sd), device)


def test_cpp_yolov9t_load_and_detect(device, tmp_path_factory, tmp_path):
    import subprocess

    model, _, path = _model(device, tmp_path_factory)
    lib_dir = ROOT / "vision.cpp_amd" / "lib"
    exe = tmp_path / "yolov9t_check"
    subprocess.run(["g++", "-std=c++20", "-O2", "-Wall", "-Wextra", "-I", str(ROOT / "include"), str(ROOT / "tests" / "cpp" / "yolov9t_check.cpp"),
                    "-o", str(exe), "-L", str(lib_dir), "-lvisioncpp", f"-Wl,-rpath,{lib_dir}"], check=True)
    w, h = 800, 600
    img = synth.images(1, w, h, seed=31)[0]
    (tmp_path / "img.raw").write_bytes(img.tobytes())
    r = subprocess.run([str(exe), str(path), str(tmp_path / "img.raw"), str(w), str(h), str(tmp_path / "out.raw")], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0 and "yolov9t-check ok" in r.stdout, (r.stdout, r.stderr)
    got = np.frombuffer((tmp_path / "out.raw").read_bytes(), vision.DETECTION_DTYPE)
    want = model.detect(img)
    assert len(want) > 0 and np.array_equal(got, want)


def test_last_split_reports_the_batch_call(device, tmp_path_factory):
    model, _, _ = _model(device, tmp_path_factory)
    imgs = synth.images(2, 256, 256, seed=4)
    model.detect_batch(imgs)
    model.detect_batch(imgs)  # replayed
    sp = model.last_split
    assert sp["device_ms"] > 0 and sp["readback_ms"] >= 0 and sp["nms_ms"] >= 0

"""YOLOv9t host code of the library (csrc/yolov9t.cpp) without a GPU: visp_yolov9t_letterbox and visp_yolov9t_nms against the
numpy restatement tests/yolov9t_ref.py, their error paths, and the family staying outside visp_model_family."""
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tests"))
import yolov9t_ref  # noqa: E402
from visioncpp_amd import _lib as L  # noqa: E402
from visioncpp_amd import synth, vision  # noqa: E402


@pytest.mark.parametrize("w,h,c,size", [(1280, 720, 3, 640), (333, 517, 3, 640), (640, 640, 3, 640), (200, 120, 4, 640), (97, 61, 3, 256),
                                        (100, 300, 4, 128)])
def test_letterbox_is_bit_exact(w, h, c, size):
    img = np.random.default_rng(w * h + c).integers(0, 256, (h, w, c), dtype=np.uint8)
    got, gain, pw, ph = vision.yolov9t_letterbox(img, size)
    want, wgain, wpw, wph = yolov9t_ref.letterbox(img, size)
    assert got.shape == (size, size, 3)
    assert np.array_equal(got, want)
    assert (gain, pw, ph) == (np.float32(wgain), np.float32(wpw), np.float32(wph))


def test_letterbox_rgba_ignores_alpha():
    rgb = np.random.default_rng(3).integers(0, 256, (90, 160, 3), dtype=np.uint8)
    rgba = np.concatenate([rgb, np.random.default_rng(4).integers(0, 256, (90, 160, 1), dtype=np.uint8)], -1)
    assert np.array_equal(vision.yolov9t_letterbox(rgb, 128)[0], vision.yolov9t_letterbox(rgba, 128)[0])


def _dense(seed, A=600, nc=16):
    """boxes in clusters (heavy overlap), scores with ties and many classes above the threshold."""
    rng = np.random.default_rng(seed)
    centres = rng.uniform(20, 600, (12, 2))
    cid = rng.integers(0, 12, A)
    xy = centres[cid] + rng.normal(0, 6, (A, 2))
    wh = rng.uniform(20, 80, (A, 2))
    boxes = np.concatenate([xy - wh / 2, xy + wh / 2], 1).astype(np.float32)
    scores = rng.uniform(0, 1, (A, nc)).astype(np.float32)
    scores = np.round(scores * 64) / 64  # many exact ties
    return boxes, scores.astype(np.float32)


def _as_tuples(d):
    return [(r["x1"], r["y1"], r["x2"], r["y2"], r["confidence"], int(r["class_id"])) for r in d]


@pytest.mark.parametrize("kw", [dict(), dict(conf=0.6, iou=0.3), dict(max_nms=500), dict(max_det=7, iou=0.7), dict(max_wh=0, iou=0.5),
                                dict(conf=0.0, max_nms=2000, max_det=50)])
def test_nms_matches_the_restatement(kw):
    boxes, scores = _dense(11)
    got = vision.yolov9t_nms(boxes, scores, **kw)
    p = dict(yolov9t_ref.DEFAULTS, **kw)
    want = yolov9t_ref.nms(boxes, scores, **p)
    assert len(got) == len(want) and len(got) > 0
    assert _as_tuples(got) == [tuple(np.float32(v) if i < 5 else v for i, v in enumerate(t)) for t in want]
    assert np.array_equal(got["confidence"], got["class_confidence"])
    n_cand = int((scores >= p["conf"]).sum())
    if "max_nms" in kw:
        assert n_cand > kw["max_nms"]
    if "max_det" in kw:
        assert len(got) == kw["max_det"]


def test_nms_refuses_bad_thresholds():
    boxes, scores = _dense(1, 20, 8)
    with pytest.raises(L.Error, match="Invalid Confidence threshold"):
        vision.yolov9t_nms(boxes, scores, conf=1.5)
    with pytest.raises(L.Error, match="Invalid IoU threshold"):
        vision.yolov9t_nms(boxes, scores, iou=-0.1)
    assert len(vision.yolov9t_nms(boxes, np.zeros_like(scores))) == 0


def test_nms_defaults_are_the_cli_values():
    p = vision._nms_params()
    assert (round(p.conf, 6), round(p.iou, 6), p.max_det, p.max_nms, p.max_wh) == (0.25, 0.45, 300, 30000, 640)


def test_yolov9t_is_not_a_model_family(tmp_path):
    path = synth.write_yolov9t_gguf(tmp_path / "y.gguf", seed=0)
    v = C.c_int32(-1)
    api = L.get_lib()
    ok = api.visp_model_detect_family(str(path).encode(), C.byref(v))
    assert ok == 0 or v.value == vision.Arch.unknown.value
    assert [s for s in L.C_API_SYMBOLS if s.startswith("visp_yolov9t_")] and all(hasattr(api, s) for s in L.C_API_SYMBOLS)


def test_scale_boxes_matches_the_restatement_and_clamps():
    rng = np.random.default_rng(8)
    n = 200
    xy = rng.uniform(-80, 720, (n, 2))
    wh = rng.uniform(1, 300, (n, 2))
    d = np.zeros(n, vision.DETECTION_DTYPE)
    d["x1"], d["y1"], d["x2"], d["y2"] = xy[:, 0], xy[:, 1], xy[:, 0] + wh[:, 0], xy[:, 1] + wh[:, 1]
    d["confidence"] = d["class_confidence"] = rng.uniform(0.25, 1, n)
    d["class_id"] = rng.integers(0, 80, n)
    _, gain, pw, ph = vision.yolov9t_letterbox(np.zeros((720, 1280, 3), np.uint8), 640)
    got = vision.yolov9t_scale_boxes(d, 1280, 720, gain, pw, ph)
    want = yolov9t_ref.scale_boxes(_as_tuples(d), 1280, 720, gain, pw, ph)
    assert [tuple(np.float32(v) for v in t[:4]) for t in want] == [(r["x1"], r["y1"], r["x2"], r["y2"]) for r in got]
    assert np.array_equal(got[["confidence", "class_id", "class_confidence"]], d[["confidence", "class_id", "class_confidence"]])
    assert (got["x1"] == 0).any() and (got["y2"] == 720).any() and (got["x2"] == 1280).any()
    assert got["x1"].min() >= 0 and got["y2"].max() <= 720
    with pytest.raises(L.Error, match="gain"):
        vision.yolov9t_scale_boxes(d, 1280, 720, 0.0, pw, ph)

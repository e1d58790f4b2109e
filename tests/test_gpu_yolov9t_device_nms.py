"""YOLOv9t's device NMS through the public interface: the bytes of the host path (the switch off), synthetic model, S = 256, batch 3."""
import ctypes as C

import numpy as np
import pytest

from tests import gpu_util as G
from visioncpp_amd import _lib as L
from visioncpp_amd import synth, vision

pytestmark = pytest.mark.gpu
_release = G.release_fixture()


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    path = synth.write_yolov9t_gguf(tmp_path_factory.mktemp("yolo_nms") / "y0.gguf", sd=synth.yolov9t_state_dict(0))
    return vision.Yolov9t.load(path, vision.Device.init(vision.Backend.gpu))


# measured: 27, 22, 26 detections at conf 0.25, none at 0.4 (that case compares empty lists and untouched rows); the third case has a max_det that cuts
@pytest.mark.parametrize("kw", [{}, dict(conf=0.4, iou=0.3, max_det=20), dict(iou=0.3, max_det=10)], ids=["defaults", "conf0.4-iou0.3-max_det20", "iou0.3-max_det10"])
def test_resident_detections_equal_the_host_path(model, kw):
    imgs = synth.images(3, 256, 256, seed=21)
    want = model.detect_batch(imgs, **kw)
    assert all(len(w) > 0 for w in want) or "conf" in kw, [len(w) for w in want]
    max_det, stream = kw.get("max_det", 300), C.c_void_p()
    L.vx_check(G.api().vx_stream_create(C.byref(stream)))
    src, counts, out = G.dev(imgs), G.dev(np.full(3, -1, np.int32)), G.dev(np.full((3, max_det, 7), 0x5A5A5A5A, np.int32))
    for call in ("first", "replayed"):
        model.detect_batch_resident(src.ptr, 3, 3, 256, out.ptr, counts.ptr, stream=stream, **kw)
        L.vx_check(G.api().vx_stream_sync(stream))
        n, rows = counts.to_numpy(np.int32, (3,)), out.to_numpy(np.int32, (3, max_det, 7))
        for b in range(3):
            assert n[b] == len(want[b]) and np.array_equal(rows[b, :n[b]], want[b].view(np.int32).reshape(-1, 7)) and np.all(rows[b, n[b]:] == 0x5A5A5A5A), (call, b)
    L.vx_check(G.api().vx_stream_destroy(stream))


def test_the_switch_changes_no_detection(model):
    imgs, photo = synth.images(3, 256, 256, seed=5), synth.images(1, 1280, 720, seed=77)[0]
    runs = [lambda: model.detect_batch(imgs), lambda: model.detect_batch(imgs, iou=0.3, max_det=10), lambda: [model.detect(photo)],
            lambda: model.detect_batch(imgs, max_det=5000)]  # above the kernel's 4096 rows: the host path answers
    want = [run() for run in runs]
    model.set_device_nms(True)
    try:
        got, host_nms_ms = [], []
        for run in runs:
            got.append(run())
            host_nms_ms.append(model.last_split["nms_ms"])
    finally:
        model.set_device_nms(False)
    assert all(len(d) > 0 for w in want for d in w) and host_nms_ms[:3] == [0, 0, 0] and host_nms_ms[3] > 0  # only the last run took the host NMS
    for w, g in zip(want, got):
        assert len(w) == len(g) and all(np.array_equal(a, b) for a, b in zip(w, g))

"""-m gpu: the timing and capture layer every model family shares (csrc/model.h) through each family's C accessors.

For every family one compute on a small fixture gives a per-group timing table whose row names, order, launch counts, FLOPs and
bytes must equal the ones recorded in tests/golden/timing_tables.json (ms is not compared); one capture reads back through the
family's read_capture (a capacity-0 size query, then the full read) with its recorded shape; and every other family's
read_timing refuses the handle with the recorded message. record(path) writes that file on a GPU host."""
import ctypes as C
import dataclasses
import json
import tempfile
from pathlib import Path

import numpy as np
import pytest

from visioncpp_amd import _lib as L
from visioncpp_amd import synth, vision

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).resolve().parent / "golden" / "timing_tables.json"
PREFIX = {"depthany": "visp_depthany_", "esrgan": "visp_esrgan_", "migan": "visp_migan_", "sam": "visp_sam_", "swin": "visp_swin_",
          "yolov9t": "visp_yolov9t_"}


def _depthany(dev, tmp, timing):
    m = vision.Model.load(synth.write_gguf(tmp / "mini.gguf", synth.MINI, seed=4), dev)
    batch = 8 if timing == 2 else 2  # 8: two sub-batches, timed per stream
    imgs = synth.images(batch, 112, 112, seed=12)
    return m, "depthany", lambda: m.compute_batch(imgs), "tokens"


def _esrgan(dev, tmp):
    m = vision.Model.load(synth.write_esrgan_gguf(tmp / "esrgan_tiny.gguf", synth.ESRGAN_TINY, seed=7), dev)
    imgs = synth.images(1, 72, 56, seed=5)
    return m, "esrgan", lambda: m.upscale_batch(imgs), None


def _migan(dev, tmp):
    m = vision.Migan.load(synth.write_migan_gguf(tmp / "migan16.gguf", 16, sd=synth.migan_state_dict(16, 1024, 128, seed=2)), dev)
    imgs = synth.images(2, 16, 16, seed=3)
    masks = np.zeros((2, 16, 16), np.uint8)
    masks[:, 4:10, 5:9] = 255
    return m, "migan", lambda: m.compute_batch(imgs, masks), "enc.out"


def _sam(dev, tmp):
    m = vision.Model.load(synth.write_tinyvit_gguf(tmp / "tinyvit.gguf", synth.TINYVIT_5M, seed=1), dev)
    imgs = synth.images(1, 1024, 1024, seed=77)
    return m, "sam", lambda: m.sam_encode_batch(imgs), "layer_3"


def _swin(dev, tmp):
    m = vision.SwinEncoder.load(synth.write_swin_gguf(tmp / "swin_mini.gguf", synth.SWIN_MINI, seed=5), dev)
    imgs = synth.images(2, 256, 288, seed=11)
    return m, "swin", lambda: m.encode_batch(imgs), "block_1_1"


def _birefnet(dev, tmp):
    cfg = dataclasses.replace(synth.SWIN_MINI, image_size=256)
    m = vision.Model.load(synth.write_birefnet_gguf(tmp / "birefnet_mini.gguf", cfg, seed=6), dev)
    imgs = synth.images(1, 192, 128, seed=21)
    return m, "swin", lambda: m.segment_batch(imgs), "squeeze"


def _yolov9t(dev, tmp):
    m = vision.Yolov9t.load(synth.write_yolov9t_gguf(tmp / "yolov9t.gguf", seed=3), dev)
    imgs = synth.images(2, 640, 640, seed=9)
    return m, "yolov9t", lambda: m.detect_batch(imgs), "model.13"


CASES = {
    "depthany": (lambda d, t: _depthany(d, t, 1), 1),
    "depthany_split": (lambda d, t: _depthany(d, t, 2), 2),
    "esrgan": (_esrgan, 1),
    "migan": (_migan, 1),
    "sam": (_sam, 1),
    "swin": (_swin, 1),
    "birefnet": (_birefnet, 1),
    "yolov9t": (_yolov9t, 1),
}


def _read_capture(m, prefix, name):
    f = getattr(m._api, prefix + "read_capture")
    n, shape = C.c_int64(), (C.c_int64 * 4)()
    L.check(f(m._handle, name.encode(), None, 0, C.byref(n), shape))
    size = [int(s) for s in shape]
    assert n.value == int(np.prod(size)), (n.value, size)
    out = np.full(n.value, np.nan, np.float32)
    n2, shape2 = C.c_int64(), (C.c_int64 * 4)()
    L.check(f(m._handle, name.encode(), out.ctypes.data, n.value, C.byref(n2), shape2))
    assert n2.value == n.value and [int(s) for s in shape2] == size
    assert np.isfinite(out).all(), name
    return size


def _foreign_errors(m, own):
    """What each other family's read_timing says about this handle."""
    errs = {}
    for fam, prefix in PREFIX.items():
        if fam == own:
            continue
        arr, n = (L.Timing * 4)(), C.c_int32()
        if getattr(m._api, prefix + "read_timing")(m._handle, arr, 4, C.byref(n)):
            errs[fam] = None
        else:
            errs[fam] = m._api.visp_get_last_error().decode()
    if own == "swin":  # a SWIN encoder handle is not a whole BiRefNet
        w, h = C.c_int32(), C.c_int32()
        ok = m._api.visp_birefnet_image_extent(m._handle, 64, 64, C.byref(w), C.byref(h))
        errs["birefnet"] = None if ok else m._api.visp_get_last_error().decode()
    return errs


def observe(case, dev, tmp):
    build, timing = CASES[case]
    m, prefix_key, run, capture = build(dev, tmp)
    prefix = PREFIX[prefix_key]
    m.enable_timing(timing)
    run()
    rows = m.read_timing()
    m.enable_timing(False)
    got = {"rows": [[r["name"], r["launches"], r["flops"], r["bytes"]] for r in rows], "ms": [r["ms"] for r in rows]}
    if capture:
        L.check(getattr(m._api, prefix + "enable_captures")(m._handle, 1))
        run()
        got["capture"] = [capture, _read_capture(m, prefix, capture)]
        L.check(getattr(m._api, prefix + "enable_captures")(m._handle, 0))
    got["foreign"] = _foreign_errors(m, prefix_key)
    del m
    return got


@pytest.fixture(scope="module")
def device():
    return vision.Device.init(vision.Backend.gpu)


@pytest.mark.parametrize("case", list(CASES))
def test_timing_table_capture_and_family_checks(case, device, tmp_path):
    want = json.loads(GOLDEN.read_text())[case]
    got = observe(case, device, tmp_path)
    names = [r[0] for r in got["rows"]]
    assert "end" not in names
    assert len(set(names)) == len(names), names
    assert names == [r[0] for r in want["rows"]]
    assert got["rows"] == want["rows"]
    assert all(ms >= 0 for ms in got["ms"])
    assert got.get("capture") == want.get("capture")
    assert got["foreign"] == want["foreign"]


def record(path):
    d = vision.Device.init(vision.Backend.gpu)
    table = {}
    for c in CASES:
        with tempfile.TemporaryDirectory() as td:
            table[c] = observe(c, d, Path(td))
        del table[c]["ms"]
        print(c, len(table[c]["rows"]), "rows", flush=True)
    Path(path).write_text("{\n" + ",\n".join(f"{json.dumps(c)}: {json.dumps(v)}" for c, v in table.items()) + "\n}\n")

"""vx_yolo_nms (csrc/kernels_yolo_nms.hip) against the host's visp_yolov9t_nms on the same candidates (small cases: tests/yolov9t_ref.nms too): every word and
count equal, guard rows untouched, no tolerance. Lists are handed over shuffled; boxes are clusters of jittered boxes on a 64-pixel canvas."""
import numpy as np
import pytest

from tests import gpu_util as G
from tests import yolov9t_ref as R
from visioncpp_amd import _lib as L
from visioncpp_amd import vision

pytestmark = pytest.mark.gpu
_release = G.release_fixture()

NC, GUARD, FILL = 3, 8, 0x5A5A5A5A


def _scene(seed, n, A, levels=0):
    """boxes f32 [A, 4], and n distinct (anchor, class) candidates in random order with scores in (0, 1], `levels` > 0: that many distinct values"""
    rng = np.random.default_rng(seed)
    c = rng.uniform(8, 40, (4, 2))[rng.integers(0, 4, A)] + rng.normal(0, 3, (A, 2))
    boxes = np.concatenate([c, c + rng.uniform(4, 24, (A, 2))], 1).astype(np.float32)
    idx = rng.choice(A * NC, n, replace=False).astype(np.int32)
    s = rng.integers(1, levels + 1, n) / levels if levels else rng.uniform(0.05, 1, n)
    return boxes, idx, s.astype(np.float32)


def _chain(fillers):
    """a suppresses b, b would suppress c, a leaves c alone: c stays. `fillers` better boxes far away come first (254: b and c fall into different rounds)"""
    boxes = np.array([[0, 100, 10, 110], [3, 100, 13, 110], [6, 100, 16, 110]] + [[70 * (i + 1), 0, 70 * (i + 1) + 9, 9] for i in range(fillers)], np.float32)
    s = np.array([0.5, 0.4, 0.3] + [0.9] * fillers, np.float32)
    p = np.random.default_rng(fillers).permutation(len(s))
    return boxes, (np.arange(len(s), dtype=np.int32) * NC + 1)[p], s[p]


def _degenerate():
    boxes, idx, s = _scene(11, 60, 32, levels=4)
    boxes[1], boxes[2], boxes[3], boxes[4], boxes[5] = boxes[0], (5, 5, 5, 9), (5, 5, 5, 9), (9, 5, 4, 9), (9, 5, 4, 9)  # duplicates, zero area, x2 < x1
    return boxes, idx, s


def _scenes(ns, seed=0, levels=0):
    return [_scene(seed + i, n, max(ns) // 2 + 2, levels) for i, n in enumerate(ns)]

CASES = [pytest.param(_scenes((n,), seed=n), {}, id=f"n{n}") for n in (0, 1, 2, 63, 64, 65, 255, 256, 257, 700)]
CASES += [pytest.param(_scenes((300,), 1, levels=8), kw, id="ties-" + "-".join(f"{k}{v}" for k, v in kw.items()))
          for kw in [{}] + [dict(max_nms=v) for v in (1, 100)] + [dict(iou=v) for v in (0.0, 0.45, 1.0)] + [dict(max_wh=v) for v in (0, 32, 640)]]
CASES += [pytest.param(_scenes((700,), 2), dict(max_det=v, iou=0.8), id=f"max_det{v}") for v in (1, 5, 64, 65, 300)]
CASES += [pytest.param([_chain(f)], {}, id=f"chain-{f}-fillers") for f in (0, 254)]
CASES += [pytest.param([_degenerate()], {}, id="degenerate"), pytest.param(_scenes((0, 257, 5), 3, levels=8), {}, id="batch-0-257-5")]


@pytest.mark.parametrize("images, kw", CASES)
def test_device_nms_equals_the_host_nms(images, kw):
    p = dict(dict(iou=0.45, max_det=300, max_nms=30000, max_wh=640), **kw)
    B, A = len(images), len(images[0][0])
    idx, score = np.zeros((B, A * NC), np.int32), np.zeros((B, A * NC), np.float32)
    want = []
    for b, (boxes, i, s) in enumerate(images):
        idx[b, :len(i)], score[b, :len(i)] = i, s
        dense = np.zeros(A * NC, np.float32)
        dense[i] = s
        want.append(vision.yolov9t_nms(boxes, dense.reshape(A, NC), conf=float(s.min()) if len(s) else 1.0, **p))
        if len(i) <= 65:
            assert [tuple(r)[:6] for r in want[b]] == R.nms(boxes, dense.reshape(A, NC), conf=s.min() if len(s) else 1.0, **p)
    rows = B * p["max_det"]
    out, counts = G.dev(np.full((rows + GUARD) * 7, FILL, np.int32)), G.dev(np.full(B + GUARD, FILL, np.int32))
    nbytes = G.api().vx_yolo_nms_workspace_bytes(B, A, NC, p["max_nms"])
    L.vx_check(G.api().vx_yolo_nms(G.ptr(np.stack([im[0] for im in images])), G.ptr(np.array([len(im[1]) for im in images], np.int32)), G.ptr(idx), G.ptr(score),
                                   B, A, NC, p["iou"], p["max_det"], p["max_nms"], p["max_wh"], G.empty(nbytes).ptr, nbytes, out.ptr, counts.ptr, None))
    G.sync()
    got, n = out.to_numpy(np.int32, (rows + GUARD, 7)), counts.to_numpy(np.int32, (B + GUARD,))
    print("kept", n[:B], "of", [len(im[1]) for im in images])
    assert n[:B].tolist() == [len(w) for w in want] and np.all(n[B:] == FILL) and np.all(got[rows:] == FILL)
    for b in range(B):
        mine = got[b * p["max_det"]:(b + 1) * p["max_det"]]
        assert np.array_equal(mine[:n[b]], want[b].view(np.int32).reshape(-1, 7)) and np.all(mine[n[b]:] == FILL)

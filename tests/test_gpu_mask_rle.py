"""vx_mask_rle_u8 (csrc/kernels_rle.hip) through vision.mask_to_rle_device against tests/rle_ref.py, on whole buffers: every row EQUALS the reference up to
min(n_runs, run_stride) and keeps its canary behind that; n_runs is the true count. Extents around the kernel's 64 x 64 tile; w a multiple of 16 on an aligned
base takes its 16-byte path (64 x 64, 80 x 130, 16 x 300, 48 x 1500), everything else its byte path. h above 256 gives a strip more than one group of four
segments (16 x 300: 2, 20 x 520: 3, 48 x 1500: 6); 48 x 1500 has 1152 boundary words, two rounds of the scan, whose carried count and position then meet every
content. The contents are rle_cases.named_masks."""
from functools import lru_cache

import numpy as np
import pytest

from tests import gpu_util as G
from tests import rle_cases as RC
from tests import rle_ref as RR

pytestmark = pytest.mark.gpu

CANARY = 0x7A7A7A7A
EXTENTS = [(1, 1), (1, 70), (70, 1), (64, 64), (63, 65), (65, 63), (130, 67), (200, 129), (80, 130), (16, 300), (20, 520), (48, 1500)]
NAMES = ["zero", "full", "first", "last", "checker", "edges", "disc", "random"]
_release_buffers = G.release_fixture()


@lru_cache(maxsize=None)
def reference(w, h):
    """-> (masks u8 [8, h, w] in the order of NAMES, their reference counts), computed once per extent"""
    cases = RC.named_masks(w, h)
    masks = np.stack([cases[k] for k in NAMES])
    return masks, [RR.mask_to_rle(m)["counts"] for m in masks]


def encode(masks, run_stride, counts=None, offset=0):
    """masks u8 [n, h, w] at `offset` bytes into their buffer -> (runs u32 [n, run_stride] or None for the count-only form, n_runs i32 [n])"""
    from visioncpp_amd import vision
    n, h, w = masks.shape
    md = G.dev(np.concatenate([np.zeros(offset, np.uint8), masks.reshape(-1)]))
    rd = G.dev(np.full(n * run_stride, CANARY, np.uint32)) if run_stride else None
    nd = G.dev(np.full(n, CANARY, np.int32))
    cd = G.dev(np.array([counts, 12345], np.int32)) if counts is not None else None
    vision.mask_to_rle_device(md.ptr + offset, n, w, h, rd.ptr if rd else None, run_stride, nd.ptr, cd.ptr if cd else None)
    return rd.to_numpy(np.uint32, (n, run_stride)) if rd else None, nd.to_numpy(np.int32, (n,))


def assert_rows(runs, n_runs, wants, run_stride, live):
    for b, want in enumerate(wants):
        if b >= live:
            assert n_runs[b] == CANARY and (runs[b] == CANARY).all(), f"mask {b} behind the count was touched"
            continue
        k = min(len(want), run_stride)
        assert n_runs[b] == len(want), (b, n_runs[b], len(want))
        assert runs[b, :k].tolist() == want[:k], f"mask {b}"
        assert (runs[b, k:] == CANARY).all(), f"mask {b}: written behind its runs"


@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "offset1"])
@pytest.mark.parametrize("w, h", EXTENTS, ids=[f"{w}x{h}" for w, h in EXTENTS])
def test_rle_equals_the_reference(w, h, offset):
    masks, wants = reference(w, h)
    stride = w * h + 3
    runs, n_runs = encode(masks, stride, offset=offset)
    assert_rows(runs, n_runs, wants, stride, len(masks))
    assert n_runs[NAMES.index("checker")] == w * h + 1  # the maximum
    _, counted = encode(masks, 0, offset=offset)
    assert counted.tolist() == n_runs.tolist(), "the count-only form"
    # three masks with a device count of 2, and a run_stride below the run count of the second
    pick = [NAMES.index(k) for k in ("random", "checker", "disc")]
    short = max(1, (w * h + 1) // 2)
    runs, n_runs = encode(masks[pick], short, counts=2, offset=offset)
    assert_rows(runs, n_runs, [wants[i] for i in pick], short, 2)


@pytest.mark.parametrize("w, h", EXTENTS, ids=[f"{w}x{h}" for w, h in EXTENTS])
def test_round_trip_and_the_host_entry(w, h):
    from visioncpp_amd import vision
    masks, wants = reference(w, h)
    rles = vision.mask_to_rle(masks)
    assert rles == [{"size": [h, w], "counts": c} for c in wants]
    for m, r in zip(masks, rles):
        assert np.array_equal(vision.rle_to_mask(r), m != 0)
    assert vision.mask_to_rle(masks[6] != 0) == rles[6]  # one bool mask -> one dict

"""kernels_rle_decode.hip against tests/rle_decode_ref.py, by equality on whole buffers (tests/buffer_check.py): decode through vision.rle_decode_device, the two
ways to the bit words through their launchers, the IoU matrix through vision.mask_iou. Extents around the 64 x 64 tile: 64 x 64 one tile on the 16-byte path,
80 x 130 a ragged last segment and a second strip, the same on a base one byte off and 37 x 53 on the byte path, 1 x 1, 1 x 200, 200 x 1, and 130 x 64 with h
exactly one segment. The contents are rle_cases.named_masks, all eight as one batch."""
from functools import lru_cache

import numpy as np
import pytest

from tests import buffer_check as BC
from tests import gpu_util as G
from tests import rle_cases as RC
from tests import rle_decode_ref as DR
from tests import rle_ref as RR
from tests import sam_select_ref as R
from visioncpp_amd import _lib as L

pytestmark = pytest.mark.gpu

CANARY, GUARD, UNSET = 0x7A, 64, -7
EXTENTS = [(64, 64, 0), (80, 130, 0), (80, 130, 1), (37, 53, 0), (1, 1, 0), (1, 200, 0), (200, 1, 0), (130, 64, 0)]
_release_buffers = G.release_fixture()


@lru_cache(maxsize=None)
def reference(w, h):
    """-> (masks u8 [8, h, w], their counts by the encoder's definition), computed once per extent"""
    masks = np.stack(list(RC.named_masks(w, h).values()))
    return masks, [RR.mask_to_rle(m)["counts"] for m in masks]


def decode(rows, w, h, value, offset=0, counts=None):
    """rows of counts -> (the buffer before: CANARY where masks go, 0 in front and in the guard; the buffer after; status i32 [n]; area i64 [n])"""
    from visioncpp_amd import vision
    n, (offsets, runs) = len(rows), DR.csr(rows)
    before = np.zeros(offset + n * h * w + GUARD, np.uint8)
    before[offset:offset + n * h * w] = CANARY
    md, rd, od, sd, ad = G.dev(before), G.dev(runs), G.dev(offsets), G.dev(np.full(n, UNSET, np.int32)), G.dev(np.full(n, UNSET, np.int64))
    cd = G.dev(np.array([counts, 12345], np.int32)) if counts is not None else None
    vision.rle_decode_device(rd.ptr, od.ptr, n, w, h, md.ptr + offset, value, cd.ptr if cd else None, sd.ptr, ad.ptr)
    return before, md.to_numpy(np.uint8, before.shape), sd.to_numpy(np.int32, (n,)), ad.to_numpy(np.int64, (n,))


def assert_decoded(run, want, value, offset, what):
    """the first len(want) masks equal want * value, every other byte of the buffer is as it was; status and area behind them likewise"""
    before, got, status, area = run
    live, px = len(want), want[0].size
    ref, written = before.astype(np.float64), np.zeros(before.shape, bool)
    ref[offset:offset + live * px] = np.concatenate([m.reshape(-1) for m in want]) * float(value)
    written[offset:offset + live * px] = True
    BC.assert_buffer(got.astype(np.float32), (ref, np.zeros(before.shape), written), what, untouched=before.astype(np.float32))
    assert (status[live:] == UNSET).all() and (area[live:] == UNSET).all(), f"{what}: status or area of a skipped mask written"


def bit_words(masks, rows, w, h, offset):
    """-> (words by vx_mask_to_bits_u8, words by vx_rle_to_bits) of the same masks, whole buffers over a fill"""
    api, n = G.api(), len(rows)
    fill = np.full(n * api.vx_mask_rle_workspace_bytes(w, h, 1) // 8, 0x5A5A5A5A5A5A5A5A, np.uint64)
    (offsets, runs), wa, wb = DR.csr(rows), G.dev(fill), G.dev(fill)
    md, rd, od = G.dev(np.concatenate([np.zeros(offset, np.uint8), masks.reshape(-1)])), G.dev(runs), G.dev(offsets)
    ws = api.vx_rle_to_bits_workspace_bytes(len(runs), n)
    L.vx_check(api.vx_mask_to_bits_u8(md.ptr + offset, n, w, h, None, 0, wa.ptr, None))
    L.vx_check(api.vx_rle_to_bits(rd.ptr, od.ptr, len(runs), n, w, h, None, 0, wb.ptr, None, None, G.empty(ws).ptr, ws, None))
    G.sync()
    return wa.to_numpy(np.uint64, fill.shape), wb.to_numpy(np.uint64, fill.shape), fill


@pytest.mark.parametrize("w, h, offset", EXTENTS, ids=[f"{w}x{h}+{o}" for w, h, o in EXTENTS])
def test_decode_and_bit_words_equal_the_reference(w, h, offset):
    masks, rows = reference(w, h)
    want = [DR.decode(r, w, h) for r in rows]
    for value in (1, 255):
        run = decode(rows, w, h, value, offset)
        assert_decoded(run, [m for m, _, _ in want], value, offset, f"decode {w}x{h} value {value}")
        assert run[2].tolist() == [0] * 8 and run[3].tolist() == [a for _, a, _ in want] == (masks != 0).sum((1, 2)).tolist()
    assert decode(rows, w, h, 255, offset)[1].tobytes() == run[1].tobytes(), "the second call gave other bytes"
    assert_decoded(decode(rows, w, h, 255, offset, counts=3), [m for m, _, _ in want[:3]], 255, offset, f"decode {w}x{h} with a device count of 3")
    from_masks, from_runs, fill = bit_words(masks, rows, w, h, offset)
    S, per = (h + 63) // 64, len(fill) // 8
    padded = np.zeros((8, S * 64, w), np.uint8)
    padded[:, :h] = masks != 0
    bits = np.packbits(padded.transpose(0, 2, 1), axis=-1, bitorder="little").reshape(8, w * S * 8).view(np.uint64)  # word (x, s) at x * S + s, bit r row 64 s + r
    expect = fill.reshape(8, per).copy()
    expect[:, :w * S] = bits
    assert np.array_equal(from_masks.reshape(8, per), expect) and np.array_equal(from_runs, from_masks)


def test_short_and_long_rows_take_the_defined_clamp(w=80, h=130):
    rows = [[100, 200, 300], [5000, 5000, 5000, 77], [0, 10, 0, 0, 20, w * h - 30], [3 * w * h], [7, 2 ** 32 - 1, 2 ** 32 - 1, 5]]
    want = [DR.decode(r, w, h) for r in rows]
    run = decode(rows, w, h, 255)
    assert_decoded(run, [m for m, _, _ in want], 255, 0, "malformed rows")
    assert run[2].tolist() == [s for _, _, s in want] == [1, 2, 0, 2, 2] and run[3].tolist() == [a for _, a, _ in want]


@pytest.mark.parametrize("w, h", [(80, 130), (37, 53)])
def test_iou_matrix_equals_the_reference(w, h):
    from visioncpp_amd import vision
    masks, rows = reference(w, h)
    rles = [{"size": [h, w], "counts": r} for r in rows]
    crowd = np.zeros(8, bool)
    crowd[[1, 6]] = True
    inter, den, _ = DR.iou(masks != 0, masks != 0, crowd)
    assert (den == 0).any() and inter.max() < 2 ** 24 and den.max() < 2 ** 24  # both operands of the division are exact in float32
    want = np.where(den > 0, inter.astype(np.float32) / np.maximum(den, 1).astype(np.float32), np.float32(0))
    for a, b in ((rles, masks), (masks, rles)):
        iou, got_inter = vision.mask_iou(a, b, crowd, return_intersection=True)
        assert np.array_equal(got_inter, inter)
        ulps = np.abs(iou.view(np.int32).astype(np.int64) - want.view(np.int32))
        print(f"iou {w}x{h}: largest distance from float32(inter) / float32(den) {ulps.max()} ulp")
        assert ulps.max() <= 1 and (iou[den == 0] == 0).all()
    # the launcher with device counts of 3 rows and 5 columns: the rest of both outputs stays as it was
    api, (words, _, _) = G.api(), bit_words(masks, rows, w, h, 0)
    wd, ca, cb = G.dev(words), G.dev(np.array([3], np.int32)), G.dev(np.array([5], np.int32))
    out_iou, out_inter, ws = G.dev(np.full(64, -1, np.float32)), G.dev(np.full(64, UNSET, np.int32)), api.vx_bitmask_iou_workspace_bytes(8, 8)
    L.vx_check(api.vx_bitmask_iou(wd.ptr, 8, wd.ptr, 8, w, h, ca.ptr, cb.ptr, None, out_inter.ptr, out_iou.ptr, G.empty(ws).ptr, ws, None))
    G.sync()
    cut = np.full((8, 8), UNSET, np.int64)
    cut[:3, :5] = DR.iou(masks != 0, masks != 0)[0][:3, :5]
    assert np.array_equal(out_inter.to_numpy(np.int32, (8, 8)), cut) and (out_iou.to_numpy(np.float32, (8, 8))[cut == UNSET] == -1).all()


def test_generated_records_decode_to_the_generated_masks(tmp_path):
    """the scenario of tests/test_gpu_sam_autogen.py: the RLE form of a generate call, decoded, is the binary form of the same call"""
    from visioncpp_amd import synth, vision
    cfg = synth.TINYVIT_5M
    path = synth.write_mobile_sam_gguf(tmp_path / "mobile_sam.gguf", cfg, enc_sd=synth.tinyvit_state_dict(cfg, R.SCENARIO_ENCODER_SEED), dec_sd=R.scenario_decoder_state_dict())
    model = vision.Model.load(path, vision.Device.init(vision.Backend.gpu))
    model.sam_set_prompt_chunk(8)
    model.sam_encode(synth.images(1, 1024, 1024, seed=R.SCENARIO_IMAGE_SEED)[0])
    kw = dict(prompts=R.scenario_prompts(), pred_iou_thresh=-float("inf"), stability_thresh=-float("inf"), nms_iou_thresh=0.9, max_masks=12)
    masks, records = model.sam_generate_masks_raw(**kw)[0], model.sam_generate_masks_rle_raw(**kw)[0]
    assert len(records) == len(masks) >= 2 and masks.any()
    assert vision.rle_decode(records, value=255).tobytes() == masks.tobytes()
    assert vision.rle_area(records).tolist() == (masks != 0).sum((1, 2)).tolist()

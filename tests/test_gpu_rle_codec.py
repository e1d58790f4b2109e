"""kernels_rle_codec.hip against tests/rle_codec_ref.py, by equality: the two launchers on synthetic run rows (count pass, write pass, guards, a second call), the
chained masks -> strings entry and the way back on rle_cases.named_masks, the four malformed kinds, and the generate call with strings out."""
import numpy as np
import pytest

from tests import gpu_util as G
from tests import rle_cases as RC
from tests import rle_codec_ref as ref
from tests import rle_ref as RR
from tests import sam_select_ref as R
from tests.test_rle_codec_ref_cpu import MALFORMED
from visioncpp_amd import _lib as L

pytestmark = pytest.mark.gpu

CANARY, GUARD, UNSET = 0x7A, 64, -7
_release_buffers = G.release_fixture()


def _row(rng, n):
    """n counts below 2^31 of every magnitude, so that the deltas take every width in both signs"""
    return (rng.integers(0, 2 ** 31, n) >> rng.integers(0, 31, n)).tolist()


def _widths():
    """one chain that climbs by the largest k-byte delta and falls by the smallest, k = 1 .. 7, on both parities"""
    cur, chain = 0, []
    for k in range(1, 8):
        cur += min(2 ** (5 * k - 1) - 1, 2 ** 31 - 1 - cur)
        chain.append(cur)
        cur -= min(cur, 2 ** (5 * k - 1))
        chain.append(cur)
    return [3, 0, 0] + [v for c in chain for v in (c, c)]


def _cases():
    rng = np.random.default_rng(11)
    mixed = [_row(rng, int(n)) for n in rng.choice([0, 0, 1, 2, 5, 70, 300, 1500], 300)]
    seams = [_row(rng, n) for n in (63, 64, 65, 127, 129, 4097)]
    return {"short": ([_row(rng, n) for n in range(6)], None), "seams": (seams, None), "widths": ([_widths()], None), "mixed300": (mixed, None), "cut": (seams, 4)}


CASES = _cases()


def csr(rows, dtype):
    offsets = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    return offsets, np.concatenate([np.asarray(r, dtype) for r in rows] + [np.zeros(1, dtype)])  # an address also without entries


def codec(rows, counts, base):
    """the rows through both launchers, each count-then-write, the packed outputs `base` bytes (runs) off a 256-byte boundary behind GUARD entries of fill
    -> (string sizes, strings buffer, run sizes, status, runs buffer)"""
    api, n = G.api(), len(rows)
    live = n if counts is None else counts
    offsets, runs = csr(rows, np.uint32)
    rd, od = G.dev(runs), G.dev(offsets)
    cd = G.dev(np.array([counts, 12345], np.int32)).ptr if counts is not None else None
    ws = api.vx_rle_compress_workspace_bytes(int(offsets[-1]), n)
    wd, sd = G.empty(ws), G.dev(np.full(n, UNSET, np.int32))
    longest = max(len(r) for r in rows)
    L.vx_check(api.vx_rle_compress(rd.ptr, od.ptr, int(offsets[-1]), longest, n, cd, 0, None, None, sd.ptr, wd.ptr, ws, None))
    sizes = sd.to_numpy(np.int32, (n,))
    boff = np.concatenate([[0], np.cumsum(np.where(np.arange(n) < live, sizes, 0))]).astype(np.int64)
    bd, bod = G.dev(np.full(base + int(boff[-1]) + GUARD, CANARY, np.uint8)), G.dev(boff)
    L.vx_check(api.vx_rle_compress(rd.ptr, od.ptr, int(offsets[-1]), longest, n, cd, 0, bd.ptr + base, bod.ptr, None, wd.ptr, ws, None))
    strings = bd.to_numpy(np.uint8, (base + int(boff[-1]) + GUARD,))
    # and back, from the strings the device wrote
    nd, td = G.dev(np.full(n, UNSET, np.int32)), G.dev(np.full(n, UNSET, np.int32))
    L.vx_check(api.vx_rle_decompress(bd.ptr + base, bod.ptr, n, cd, 0, None, None, nd.ptr, td.ptr, None))
    n_runs = nd.to_numpy(np.int32, (n,))
    roff = np.concatenate([[0], np.cumsum(np.where(np.arange(n) < live, n_runs, 0))]).astype(np.int64)
    out, rod = G.dev(np.full(base + int(roff[-1]) + GUARD, 0x7A7A7A7A, np.uint32)), G.dev(roff)
    L.vx_check(api.vx_rle_decompress(bd.ptr + base, bod.ptr, n, cd, 0, out.ptr + 4 * base, rod.ptr, None, td.ptr, None))
    G.sync()
    return sizes, strings, n_runs, td.to_numpy(np.int32, (n,)), out.to_numpy(np.uint32, (base + int(roff[-1]) + GUARD,))


@pytest.mark.parametrize("base", [0, 3])
@pytest.mark.parametrize("name", list(CASES))
def test_launchers_equal_the_reference(name, base):
    rows, counts = CASES[name]
    live = len(rows) if counts is None else counts
    want = [ref.enc(r) for r in rows[:live]]
    if name == "widths":
        deltas = [c - rows[0][i + 1] for i, c in enumerate(rows[0][3:])]
        width = lambda d: len(ref.enc([0, max(0, -d), 0, max(0, -d) + d])) - len(ref.enc([0, max(0, -d), 0]))  # noqa: E731
        assert {(d < 0, width(d)) for d in deltas} == {(s, k) for s in (False, True) for k in range(1, 8)}, "the case no longer holds every width in both signs"
    sizes, strings, n_runs, status, runs = codec(rows, counts, base)
    skipped = [UNSET] * (len(rows) - live)
    assert sizes.tolist() == [len(s) for s in want] + skipped and n_runs.tolist() == [len(r) for r in rows[:live]] + skipped and status.tolist() == [0] * live + skipped
    fill = bytes([CANARY])
    assert strings.tobytes() == fill * base + b"".join(want) + fill * GUARD, "the strings, or a byte around them"
    flat = np.array([c for r in rows[:live] for c in r], np.uint32)
    assert np.array_equal(runs, np.concatenate([np.full(base, 0x7A7A7A7A, np.uint32), flat, np.full(GUARD, 0x7A7A7A7A, np.uint32)])), "the runs, or a run around them"
    again = codec(rows, counts, base)
    assert again[1].tobytes() == strings.tobytes() and again[4].tobytes() == runs.tobytes(), "the second call gave other bytes"


@pytest.mark.parametrize("w, h", [(65, 63), (1, 1), (640, 480)])
def test_masks_to_strings_and_back(w, h):
    from visioncpp_amd import vision
    masks = np.stack(list(RC.named_masks(w, h).values()))
    want = [ref.enc(RR.mask_to_rle(m)["counts"]) for m in masks]
    got = vision.mask_to_coco_rle(masks)
    assert [r["counts"] for r in got] == want and all(r["size"] == [h, w] for r in got)
    assert vision.mask_to_coco_rle(masks)[7] == got[7]
    assert np.array_equal(vision.rle_decode(got, value=1), (masks != 0).astype(np.uint8))
    text = [{"size": r["size"], "counts": r["counts"].decode("ascii")} for r in got]
    assert vision.rle_area(text).tolist() == (masks != 0).sum((1, 2)).tolist() and vision.rle_compress(vision.rle_decompress(text)) == got


def test_malformed_strings_between_good_ones():
    api, good = G.api(), ref.enc([5, 3, 7, 3, 7, 2, 39])
    rows = [good] + [s for k in (1, 2, 3, 4) for s in (MALFORMED[k].encode(), good)]
    boff, data = csr([list(s) for s in rows], np.uint8)
    bd, bod, nd, td = G.dev(data), G.dev(boff), G.dev(np.full(9, UNSET, np.int32)), G.dev(np.full(9, UNSET, np.int32))
    L.vx_check(api.vx_rle_decompress(bd.ptr, bod.ptr, 9, None, 0, None, None, nd.ptr, td.ptr, None))
    n_runs = nd.to_numpy(np.int32, (9,))
    assert n_runs.tolist() == [7, 0] * 4 + [7] and td.to_numpy(np.int32, (9,)).tolist() == [0, 1, 0, 2, 0, 3, 0, 4, 0]
    roff = np.concatenate([[0], np.cumsum(n_runs)]).astype(np.int64)
    out = G.dev(np.full(35 + GUARD, 0x7A7A7A7A, np.uint32))
    L.vx_check(api.vx_rle_decompress(bd.ptr, bod.ptr, 9, None, 0, out.ptr, G.dev(roff).ptr, None, None, None))
    G.sync()
    assert out.to_numpy(np.uint32, (35 + GUARD,)).tolist() == [5, 3, 7, 3, 7, 2, 39] * 5 + [0x7A7A7A7A] * GUARD


def test_generate_call_with_strings_out(tmp_path):
    """the scenario of tests/test_gpu_sam_rle.py: each string decompresses to the uncompressed_rle counts of the same call, every other key is equal"""
    from visioncpp_amd import synth, vision
    cfg = synth.TINYVIT_5M
    path = synth.write_mobile_sam_gguf(tmp_path / "mobile_sam.gguf", cfg, enc_sd=synth.tinyvit_state_dict(cfg, R.SCENARIO_ENCODER_SEED), dec_sd=R.scenario_decoder_state_dict())
    model = vision.Model.load(path, vision.Device.init(vision.Backend.gpu))
    model.sam_set_prompt_chunk(8)
    model.sam_encode(synth.images(1, 320, 240, seed=R.SCENARIO_IMAGE_SEED)[0])
    kw = dict(prompts=R.scenario_prompts(320, 240), pred_iou_thresh=-float("inf"), stability_thresh=-float("inf"), nms_iou_thresh=0.9, max_masks=12, min_mask_region_area=40)
    plain, packed = model.sam_generate_masks(output_mode="uncompressed_rle", **kw), model.sam_generate_masks_coco_rle(**kw)
    assert len(packed) == len(plain) >= 2 and any(len(r["segmentation"]["counts"]) > 1 for r in plain)
    for a, b in zip(plain, packed):
        assert isinstance(b["segmentation"]["counts"], bytes) and b["segmentation"]["counts"] == ref.enc(a["segmentation"]["counts"])
        assert vision.rle_decompress(b["segmentation"]) == a["segmentation"] and set(a) == set(b) and all(a[k] == b[k] for k in a if k != "segmentation")

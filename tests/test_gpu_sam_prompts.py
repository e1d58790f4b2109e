"""Many prompts per sam_encode in one batched pass (Model.sam_compute_batch / visp_sam_compute_batch_*): against the CPU oracle on the GPU's own
embedding, against the single-prompt sam_compute (the same decoder with a batch of one), across chunk sizes, on a non-square image, and the error paths. The model is the
TINYVIT_5M encoder (seed 2) + decoder (seed 11) file of tests/test_gpu_tinyvit.py's sam_full, built here; one sam_encode of the seed-31 image is
shared by the tests that use it. Tolerances are those of test_decoder_matches_oracle_on_the_same_embedding."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

from oracle import oracle as O

pytestmark = pytest.mark.gpu

# three points (the third within 8 px of two borders) and two boxes, mixed
PROMPTS = [[700, 300], [200, 120, 640, 900], [5, 1019], [600, 100, 900, 300], [512, 512]]
MARGIN = 0.05  # the oracle's best of the first three leads by at least this: above twice the iou tolerance, so both sides choose the same plane


@pytest.fixture(autouse=True)
def _release():
    yield
    from tests import gpu_util as G
    G.release()


def _iou(a, b):
    a, b = a > 0, b > 0
    return (a & b).sum() / max(1, (a | b).sum())


def _assert_close(got, want, what):
    """(masks u8 [n, h, w], iou [n, 4], logits [n, 4, 256, 256]) on both sides, prompt by prompt; `want` is the reference side"""
    gm, gi, gl = got
    wm, wi, wl = want
    assert gm.shape == wm.shape and gl.shape == wl.shape and gi.shape == wi.shape
    for p in range(gm.shape[0]):
        scale = np.abs(wl[p]).mean()
        err = np.abs(gl[p] - wl[p])
        print(f"{what} prompt {p}: logit err mean {err.mean():.4f} max {err.max():.4f} (scale {scale:.3f}), iou err {np.abs(gi[p] - wi[p]).max():.4f}, "
              f"mask pixels differing {(gm[p] != wm[p]).mean():.2e}, mask IoU {_iou(gm[p], wm[p]):.5f}")
        assert err.mean() < 0.02 * scale and err.max() < 0.25 * max(1.0, np.abs(wl[p]).max()), (what, p, err.mean(), err.max(), scale)
        np.testing.assert_allclose(gi[p], wi[p], atol=0.02, err_msg=f"{what} prompt {p}")
        assert set(np.unique(gm[p])) <= {0, 255}
        assert (gm[p] != wm[p]).mean() < 5e-3 and _iou(gm[p], wm[p]) > 0.99, (what, p, (gm[p] != wm[p]).mean(), _iou(gm[p], wm[p]))


def _build(tmp, name, dec_sd=None):
    from visioncpp_amd import synth, vision
    cfg = synth.TINYVIT_5M
    enc_sd = synth.tinyvit_state_dict(cfg, 2)
    dec_sd = dec_sd if dec_sd is not None else synth.sam_decoder_state_dict(11)
    path = synth.write_mobile_sam_gguf(tmp / name, cfg, enc_sd=enc_sd, dec_sd=dec_sd)
    dev = vision.Device.init(vision.Backend.gpu)
    model = vision.Model.load(path, dev)
    model.enable_captures(True)  # keeps the logit planes for sam_read_masks / sam_read_masks_batch
    tensors, conv2d = synth.mobile_sam_gguf_tensors(enc_sd, dec_sd)
    return dict(model=model, dev=dev, path=path, om=O.Model(tensors, conv2d, "whcn"), cfg=cfg, encoded=None)


def _encode31(s):
    """the seed-31 image is the model's current embedding (a test that encodes another image resets `encoded`)"""
    from visioncpp_amd import synth
    if s["encoded"] != 31:
        s["embed"] = s["model"].sam_encode(synth.images(1, 1024, 1024, seed=31)[0])
        s["encoded"] = 31
    return s["embed"]


def _batch(s, prompts, chunk):
    m = s["model"]
    m.sam_set_prompt_chunk(chunk)
    masks, iou, chosen = m.sam_compute_batch(prompts)
    logits, iou2 = m.sam_read_masks_batch()
    np.testing.assert_array_equal(iou, iou2)
    np.testing.assert_array_equal(chosen, np.argmax(iou[:, :3], axis=1))
    return masks, iou, logits


def _single(m, prompt):
    """(mask u8 [h, w], iou [4], logits [4, 256, 256]) of one sam_compute"""
    mask = m.sam_compute(prompt)
    logits, iou = m.sam_read_masks()
    return mask, iou, logits


def _assert_same_bytes(one, alone, prompt):
    """`one` of _single against `alone`, the _batch of that prompt by itself"""
    for a, b in zip(one, alone):
        assert b.shape == (1,) + a.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes(), prompt


@pytest.fixture(scope="module")
def sam(tmp_path_factory):
    s = _build(tmp_path_factory.mktemp("samprompts"), "mobile_sam.gguf")
    embed = _encode31(s)
    # the oracle on the GPU's own embedding, once for the module
    ref = [O.sam_compute(s["om"], embed, 1024, 1024, p, return_all=True) for p in PROMPTS]
    s["oracle"] = (np.stack([r[0] for r in ref]), np.stack([r[1] for r in ref]), np.stack([r[2] for r in ref]))
    yield s
    s.pop("model")
    s.pop("dev")


@pytest.fixture(scope="module")
def chunk2(sam):
    """the five prompts in chunks of 2 + 2 + 1"""
    _encode31(sam)
    return _batch(sam, PROMPTS, 2)


def test_oracle_margins_hold_with_the_oracles_own_encoder(sam):
    """The choice of prompts: with the oracle's OWN encoder (no GPU number in it) and on the GPU's embedding alike, the best of the first three iou
    predictions leads by at least MARGIN for every prompt, so no prompt has to be left out of the mask comparisons below."""
    from visioncpp_amd import synth
    img = synth.images(1, 1024, 1024, seed=31)[0]
    mean, std = np.array([0.485, 0.456, 0.406], np.float32), np.array([0.229, 0.224, 0.225], np.float32)
    x = (img.astype(np.float32) / np.float32(255.0) - mean) / std
    cfg = sam["cfg"]
    emb = O.tinyvit_encode(sam["om"], O.tinyvit_params(cfg.img_size, cfg.layers()), x)
    for p, prompt in enumerate(PROMPTS):
        _, iou, _ = O.sam_compute(sam["om"], emb, 1024, 1024, prompt, return_all=True)
        for which, v in (("oracle encoder", iou), ("GPU embedding", sam["oracle"][1][p])):
            top = np.sort(v[:3])
            assert top[2] - top[1] >= MARGIN, (which, prompt, v)


def test_batch_matches_the_oracle_on_the_same_embedding(sam, chunk2):
    masks, iou, logits = chunk2
    assert masks.shape == (5, 1024, 1024) and masks.dtype == np.uint8 and iou.shape == (5, 4) and logits.shape == (5, 4, 256, 256)
    np.testing.assert_array_equal(np.argmax(iou[:, :3], axis=1), np.argmax(sam["oracle"][1][:, :3], axis=1))
    _assert_close(chunk2, sam["oracle"], "batch (chunk 2) against the oracle")


def test_batch_matches_the_single_prompt_call_which_keeps_its_bytes(sam, chunk2):
    m = sam["model"]
    _encode31(sam)

    def singles():
        out = []
        for p in PROMPTS:
            mask = m.sam_compute(p)
            logits, iou = m.sam_read_masks()
            out.append((mask, iou, logits))
        return np.stack([o[0] for o in out]), np.stack([o[1] for o in out]), np.stack([o[2] for o in out])

    before = singles()
    again = _batch(sam, PROMPTS, 2)
    after = singles()
    for b, a in zip(before, after):
        assert b.tobytes() == a.tobytes(), "sam_compute changed across a batch call"
    for c, a in zip(chunk2, again):
        assert c.tobytes() == a.tobytes(), "the same batch call twice gave other bytes"
    _assert_close(chunk2, before, "batch (chunk 2) against sam_compute")
    _assert_close(before, sam["oracle"], "sam_compute against the oracle")


def test_sam_compute_is_the_batch_of_one_bit_for_bit(sam):
    """sam_compute runs the one decoder with n = 1: mask, iou[4] and logits[4, 256, 256] have the bytes of sam_compute_batch with that prompt alone, for
    points and boxes (test_non_square_image_host_and_device_entries_agree: the same on a 640 x 480 image)."""
    _encode31(sam)
    for prompt in PROMPTS:
        _assert_same_bytes(_single(sam["model"], prompt), _batch(sam, [prompt], 64), prompt)


def test_chunk_sizes_and_single_prompt_batches_agree(sam, chunk2):
    """Chunk 2 against chunk 64 (one chunk of five) and each prompt alone: within the tolerances, not bit for bit -- layer 0's token -> image
    attention runs all 7 B queries of a chunk as one batch and splits its keys only up to 32 queries, so its sums change order with the chunk."""
    _encode31(sam)
    whole = _batch(sam, PROMPTS, 64)
    _assert_close(whole, chunk2, "chunk 64 against chunk 2")
    _assert_close(whole, sam["oracle"], "chunk 64 against the oracle")
    twice = _batch(sam, PROMPTS, 64)
    for a, b in zip(whole, twice):
        assert a.tobytes() == b.tobytes()
    alone = [_batch(sam, [p], 64) for p in PROMPTS]
    alone = tuple(np.concatenate([a[i] for a in alone]) for i in range(3))
    _assert_close(alone, whole, "each prompt alone against the batch of five")
    # no cross-prompt effects: the same prompt gives the same bytes whatever stands next to it in its chunk (chunk 1: every launch has one prompt's rows)
    ones = _batch(sam, PROMPTS, 1)
    for a, b in zip(ones, alone):
        assert a.tobytes() == b.tobytes()
    rev = _batch(sam, PROMPTS[::-1], 1)
    for a, b in zip(ones, rev):
        assert a.tobytes() == b[::-1].tobytes()


def test_near_tied_iou_predictions_in_a_batch(tmp_path):
    """The near-tie of tests/test_gpu_tinyvit.py (rows 0 and 1 of the iou head's last layer equal, biases 1e-4 apart) in a batch of three: the f32 head on
    the device ranks them as the oracle does, for every prompt of the batch."""
    from visioncpp_amd import synth
    dec_sd = synth.sam_decoder_state_dict(11)
    wk = [k for k in dec_sd if k.endswith("iou_prediction_head.layers.2.weight")][0]
    bk = wk.replace("weight", "bias")
    dec_sd[wk][1] = dec_sd[wk][0]
    dec_sd[wk][2] = dec_sd[wk][0]
    dec_sd[bk][1] = dec_sd[bk][0] + np.float32(1e-4)
    dec_sd[bk][2] = dec_sd[bk][0] - np.float32(0.25)
    s = _build(tmp_path, "tie.gguf", dec_sd)
    embed = _encode31(s)
    prompts = [[700, 300], [200, 120, 640, 900], [512, 512]]
    masks, iou, _ = _batch(s, prompts, 2)
    assert (iou[:, 1] > iou[:, 0]).all() and (iou[:, 0] > iou[:, 2]).all(), iou
    assert np.abs((iou[:, 1] - iou[:, 0]) - 1e-4).max() < 3e-5, iou[:, 1] - iou[:, 0]
    _, _, chosen = s["model"].sam_compute_batch(prompts)
    assert (chosen == 1).all()
    for p, prompt in enumerate(prompts):
        want, wiou, _ = O.sam_compute(s["om"], embed, 1024, 1024, prompt, return_all=True)
        assert int(np.argmax(wiou[:3])) == 1
        assert (masks[p] != want).mean() < 5e-3, (prompt, (masks[p] != want).mean())


def test_non_square_image_host_and_device_entries_agree(sam):
    from tests import gpu_util as G
    from visioncpp_amd import synth
    m = sam["model"]
    m.sam_encode(synth.images(1, 640, 480, seed=8)[0])  # [480, 640, 3]
    sam["encoded"] = None
    assert m.sam_image_extent() == (640, 480)
    prompts = [[320, 200], [100, 80, 500, 400], [630, 470]]
    m.sam_set_prompt_chunk(2)
    masks, iou, chosen = m.sam_compute_batch(prompts)
    assert masks.shape == (3, 480, 640) and set(np.unique(masks)) <= {0, 255}
    dm, di, dc = G.empty(3 * 480 * 640), G.empty(3 * 16), G.empty(3 * 4)
    m.sam_compute_batch_device(prompts, dm.ptr, di.ptr, dc.ptr)
    G.sync()
    np.testing.assert_array_equal(dm.to_numpy(np.uint8, (3, 480, 640)), masks)
    np.testing.assert_array_equal(di.to_numpy(np.float32, (3, 4)), iou)
    np.testing.assert_array_equal(dc.to_numpy(np.int32, (3,)), chosen)
    only = G.dev(np.full(3 * 480 * 640 + 64, 7, np.uint8))
    m.sam_compute_batch_device(prompts, only.ptr)  # iou and chosen may be NULL
    G.sync()
    got = only.to_numpy(np.uint8, (3 * 480 * 640 + 64,))
    np.testing.assert_array_equal(got[: 3 * 480 * 640].reshape(3, 480, 640), masks)
    assert (got[3 * 480 * 640:] == 7).all()
    kept = m.sam_read_masks_batch()  # of the batch call just made
    singles = []
    for p, prompt in enumerate(prompts):  # and the single-prompt call on the same embedding
        singles.append(_single(m, prompt))
        one = singles[-1][0]
        assert (one != masks[p]).mean() < 5e-3, (prompt, (one != masks[p]).mean())
    for a, b in zip(kept, m.sam_read_masks_batch()):  # sam_compute keeps its logits apart from the batch call's
        assert a.shape[0] == 3 and a.tobytes() == b.tobytes(), "a sam_compute in between changed the batch call's read-back"
    for prompt, one in zip(prompts, singles):
        _assert_same_bytes(one, _batch(sam, [prompt], 64), prompt)


def test_errors(sam, tmp_path):
    from visioncpp_amd import _lib as L, synth, vision
    m = sam["model"]
    _encode31(sam)
    fresh = vision.Model.load(synth.write_mobile_sam_gguf(tmp_path / "s.gguf", seed=4), m._device)
    with pytest.raises(L.Error, match="call sam_encode"):
        fresh.sam_compute_batch([[1, 2]])
    with pytest.raises(L.Error, match="call sam_encode"):
        fresh.sam_compute_batch_device([[1, 2]], 4096)
    with pytest.raises(L.Error, match="must be 2 or 4"):
        m.sam_compute_batch([[1, 2], [1, 2, 3]])
    with pytest.raises(L.Error, match="empty batch"):
        m.sam_compute_batch([])
    api = L.get_lib()
    p, k = vision.Model._sam_prompt_arrays([[1, 2]])
    assert api.visp_sam_compute_batch_device(m._handle, p.ctypes.data, k.ctypes.data, 1, None, None, None, None) == 0
    assert b"null" in api.visp_get_last_error()
    assert api.visp_sam_compute_batch_device(m._handle, None, k.ctypes.data, 1, 4096, None, None, None) == 0
    assert api.visp_sam_compute_batch_host(m._handle, p.ctypes.data, None, 1, 4096, None, None) == 0
    assert b"null" in api.visp_get_last_error()
    for bad in (0, 257, -1):
        with pytest.raises(L.Error, match="1 .. 256"):
            m.sam_set_prompt_chunk(bad)
    enc_only = vision.Model.load(synth.write_tinyvit_gguf(tmp_path / "t.gguf", sam["cfg"], seed=1), m._device)
    enc_only.sam_encode(synth.images(1, 64, 48, seed=3)[0])
    with pytest.raises(L.Error, match="dec"):
        enc_only.sam_compute_batch([[1, 2]])
    m.enable_captures(False)
    try:
        m.sam_compute_batch([[700, 300]])
        with pytest.raises(L.Error, match="enable captures"):
            m.sam_read_masks_batch()
    finally:
        m.enable_captures(True)


def test_cpp_overloads_of_vision_h(sam):
    """tests/cpp/sam_prompts_check.cpp: sam_compute_batch(points) and sam_compute_batch(boxes) of include/visp/vision.h against sam_compute, in a process of its own"""
    exe = Path(__file__).resolve().parents[1] / "vision.cpp_amd" / "lib" / "sam_prompts_check"
    assert exe.exists(), "build() makes it"
    r = subprocess.run([str(exe), str(sam["path"]), "320", "240"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    words = r.stdout.split()
    assert words[:3] == ["5", "masks", "320x240"], r.stdout
    assert int(words[4]) < 5e-3 * 5 * 320 * 240, r.stdout

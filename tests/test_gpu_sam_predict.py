"""Model.sam_predict (visp_sam_predict_*): SAM's SamPredictor.predict -- labelled points, a box with points, the previous low-resolution logits as mask input --
against the CPU oracle on the GPU's own embedding. The oracle's decoder takes any number of sparse tokens, built here in float64 as SAM's PromptEncoder does, and
sees the embedding only as embed + dense prompt: a mask input is embed + dense - no_mask_embed with `dense` from tests/sam_dense_ref.py. The model is the
TinyViT-5M + decoder file of tests/test_gpu_sam_prompts.py with the mask_downscaling tensors; tolerances are that module's _assert_close. One sam_encode of the
seed-31 image is shared."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import sam_dense_ref as R
from tests.test_gpu_sam_prompts import MARGIN, _assert_close, _build

pytestmark = pytest.mark.gpu

# (points, labels, box): one positive point; two positive and one negative; a box and one negative
PROMPTS = {"point": ([[700, 300]], [1], None), "three_points": ([[640, 420], [720, 330], [300, 800]], [1, 1, 0], None),
           "box_negative": ([[520, 500]], [0], [200, 120, 640, 900])}


@pytest.fixture(autouse=True)
def _release():
    yield
    from tests import gpu_util as G
    G.release()


@pytest.fixture(scope="module")
def sam(tmp_path_factory):
    from visioncpp_amd import synth
    s = _build(tmp_path_factory.mktemp("sampredict"), "mobile_sam_mask.gguf", synth.sam_decoder_state_dict(11, mask_input=True))
    s["tensors"] = synth.mobile_sam_gguf_tensors(synth.tinyvit_state_dict(s["cfg"], 2), synth.sam_decoder_state_dict(11, mask_input=True))[0]
    s["embed"] = s["model"].sam_encode(synth.images(1, 1024, 1024, seed=31)[0])
    yield s
    s.pop("model")
    s.pop("dev")


def _sparse(tensors, points, labels, box, w, h):
    """SAM's PromptEncoder._embed_points / _embed_boxes in float64 on the file's values: [k points | padding not-a-point, or the box's corners][dim]"""
    t = lambda name: tensors["prompt_encoder." + name].astype(np.float64)
    gauss, nap = t("pe_layer.positional_encoding_gaussian_matrix"), t("not_a_point_embed.weight")[0]
    label = [t(f"point_embeddings.{i}.weight")[0] for i in range(4)]

    def encode(xy):
        c = 2 * ((np.asarray(xy, np.float64) * (1024 / max(w, h)) + 0.5) / 1024) - 1
        v = 2 * np.pi * (c @ gauss)
        return np.concatenate([np.sin(v), np.cos(v)])

    rows = [nap if l < 0 else encode(p) + label[l] for p, l in zip(points, labels)]
    rows += [nap] if box is None else [encode(box[:2]) + label[2], encode(box[2:]) + label[3]]
    return np.stack(rows)


def _oracle(s, embed, prompt, mask_input, w, h):
    """(mask u8 [h, w], iou [4], logits [4, 256, 256]) of the oracle's decoder; the best of the first three must lead by MARGIN"""
    points, labels, box = prompt
    if mask_input is not None:
        dense = R.dense(mask_input[None], R.weights(s["tensors"]))[1][0]
        embed = embed.astype(np.float64) + dense - s["tensors"]["prompt_encoder.no_mask_embed.weight"].astype(np.float64)[0]
    logits, iou = O.sam_predict_masks(s["om"], embed, _sparse(s["tensors"], points, labels, box, w, h))
    top = np.sort(iou[:3])
    assert top[2] - top[1] >= MARGIN, ("the oracle's two best predictions are too close for this prompt", prompt, iou)
    return O.sam_process_mask(logits[int(np.argmax(iou[:3]))], w, h), iou, logits


def _predict(m, prompt, mask_input=None, plane=-1):
    points, labels, box = prompt
    mask, iou, chosen, low = m.sam_predict(points, labels, box, mask_input, plane)
    logits, iou2 = m.sam_read_masks_batch()
    assert iou.tobytes() == iou2[0].tobytes() and low.tobytes() == logits[0, chosen].tobytes(), "low_res_logits is not the chosen plane of the logits"
    assert chosen == (int(np.argmax(iou[:3])) if plane < 0 else plane)
    return (mask, iou, logits[0]), low


@pytest.mark.parametrize("name", list(PROMPTS))
def test_prompt_and_its_refinement_match_the_oracle(sam, name):
    """the prompt alone, then the same prompt with the first call's low-resolution logits as mask input"""
    m, low = sam["model"], None
    for round_ in ("alone", "with its mask input"):
        got, low_next = _predict(m, PROMPTS[name], low)
        want = _oracle(sam, sam["embed"], PROMPTS[name], low, 1024, 1024)
        _assert_close(tuple(a[None] for a in got), tuple(a[None] for a in want), f"{name} {round_}")
        low = low_next


def test_non_square_image_with_mask_input(sam):
    from visioncpp_amd import synth
    m = sam["model"]
    embed = m.sam_encode(synth.images(1, 640, 480, seed=8)[0])
    try:
        prompt = ([[320, 200], [500, 100]], [1, 0], None)
        _, low = _predict(m, prompt)
        got, _ = _predict(m, prompt, low)
        assert got[0].shape == (480, 640)
        _assert_close(tuple(a[None] for a in got), tuple(a[None] for a in _oracle(sam, embed, prompt, low, 640, 480)), "640 x 480 with its mask input")
    finally:
        m.sam_encode(synth.images(1, 1024, 1024, seed=31)[0])


@pytest.mark.parametrize("prompt", [[700, 300], [200, 120, 640, 900]], ids=["point", "box"])
def test_a_point_or_a_box_alone_keeps_the_bytes_of_sam_compute_batch(sam, prompt):
    m = sam["model"]
    masks, iou, chosen = m.sam_compute_batch([prompt])
    logits = m.sam_read_masks_batch()[0]
    (mask, iou2, logits2), low = _predict(m, ([prompt], [1], None) if len(prompt) == 2 else (None, None, prompt))
    assert mask.tobytes() == masks[0].tobytes() and iou2.tobytes() == iou[0].tobytes() and logits2.tobytes() == logits[0].tobytes()
    assert low.tobytes() == logits[0, chosen[0]].tobytes()
    fixed, _ = _predict(m, ([prompt], [1], None) if len(prompt) == 2 else (None, None, prompt), plane=3)  # a fixed plane changes the mask, nothing else
    assert fixed[1].tobytes() == iou2.tobytes() and fixed[2].tobytes() == logits2.tobytes()
    assert (fixed[0] != O.sam_process_mask(logits2[3], 1024, 1024)).mean() < 5e-3


def test_chunk_size_does_not_change_the_bytes_with_mask_inputs(sam):
    """five prompts with mask inputs in chunks of 2 + 2 + 1 and in one chunk: with a mask input every launch works on rows of single prompts (without one, layer 0
    shares its image side and runs all queries of a chunk as one batch: tests/test_gpu_sam_prompts.py compares that within tolerances)"""
    m = sam["model"]
    pts = np.array([[[700, 300], [300, 800]], [[640, 420], [100, 100]], [[512, 512], [900, 200]], [[200, 700], [720, 330]], [[5, 1019], [400, 400]]], np.int32)
    lab = np.tile(np.array([1, 0], np.int32), (5, 1))
    low = m.sam_predict(pts, lab)[3]
    runs = []
    for chunk in (2, 64):
        m.sam_set_prompt_chunk(chunk)
        runs.append(m.sam_predict(pts, lab, mask_input=low) + m.sam_read_masks_batch())
    for a, b in zip(*runs):
        assert a.shape[0] == 5 and a.tobytes() == b.tobytes()


def test_refusals(sam, tmp_path):
    from visioncpp_amd import _lib as L, synth, vision
    m = sam["model"]
    assert m.sam_mask_input_size() == 256
    low = np.zeros((256, 256), np.float32)
    plain = vision.Model.load(synth.write_mobile_sam_gguf(tmp_path / "plain.gguf", sam["cfg"], seed=4), m._device)
    plain.sam_encode(synth.images(1, 64, 48, seed=3)[0])
    assert plain.sam_mask_input_size() == 0
    with pytest.raises(L.Error, match="mask_downscaling"):
        plain.sam_predict([[10, 10]], mask_input=low)
    with pytest.raises(L.Error, match="side 128"):
        m.sam_predict([[10, 10]], mask_input=low[:128, :128])
    with pytest.raises(L.Error, match="label 2"):
        m.sam_predict([[10, 10]], [2])
    with pytest.raises(L.Error, match="a point or a box"):
        m.sam_predict(np.zeros((1, 0, 2), np.int32))
    for plane in (-2, 4):
        with pytest.raises(L.Error, match="-1 .. 3"):
            m.sam_predict([[10, 10]], plane=plane)

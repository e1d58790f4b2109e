"""Automatic mask generation (Model.sam_generate_masks* / visp_sam_generate_masks_*) on the synthetic full-size model of tests/test_gpu_sam_prompts.py
(TINYVIT_5M encoder seed 2, decoder seed 11 with the four biases of tests/sam_select_ref.scenario_decoder_state_dict lowered; the seed-31 image): a 4 x 4
point grid plus two boxes at chunk 8, so the chunks are 8 + 8 + 2.

With captures enabled, everything a call returns must EQUAL tests/sam_select_ref.py applied to the call's OWN captured logits and iou predictions -- the kept
list, its order, the counts and the info rows -- and the masks must be the bytes vx_sam_process_masks makes of the same planes. Comparing against the
call's own logits keeps f16 differences from the oracle out of the threshold decisions. The stability score alone may differ by 1 ulp of float32 (the
division's last bit; no decision reads it). The thresholds are midpoints between adjacent sorted captured values, chosen so that each filter rejects a
candidate, at least eight reach NMS, and NMS suppresses at least one and keeps at least two: asserted on the reference before anything is compared.
tests/test_sam_select_ref_cpu.py shows with the oracle's own encoder and decoder that such thresholds exist for this scenario."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

from tests import sam_select_ref as R

pytestmark = pytest.mark.gpu

CHUNK = 8


@pytest.fixture(autouse=True)
def _release():
    yield
    from tests import gpu_util as G
    G.release()


def _encode31(s):
    from visioncpp_amd import synth
    if s["encoded"] != 31:
        s["model"].sam_encode(synth.images(1, 1024, 1024, seed=R.SCENARIO_IMAGE_SEED)[0])
        s["encoded"] = 31


def _generate(s, prompts, thresholds, max_masks, chunk=CHUNK):
    """one host call with captures -> dict(masks, info_i32, info_f32, counts, logits f16 [n, 4, 256, 256], iou [n, 4])"""
    m = s["model"]
    m.sam_set_prompt_chunk(chunk)
    pt, st, off, nt = thresholds
    masks, ii, fi, counts = m.sam_generate_masks_raw(prompts, pred_iou_thresh=pt, stability_thresh=st, stability_offset=off, nms_iou_thresh=nt, max_masks=max_masks)
    logits, iou = m.sam_read_masks_batch()
    l16 = logits.astype(np.float16)
    assert np.array_equal(l16.astype(np.float32), logits)  # the captures are the device's f16 values
    return dict(masks=masks, info_i32=ii, info_f32=fi, counts=counts, logits=l16, iou=iou)


def _masks_by_process_masks(logits16, cands, w, h):
    """the u8 masks vx_sam_process_masks makes of the captured planes of the candidates `cands`"""
    from tests import gpu_util as G
    from visioncpp_amd import _lib as L
    n_px = 256 * 256
    src = G.dev(np.ascontiguousarray(logits16))
    sw, sh = R.scaled_extent(w, h)
    scaled, out = G.empty(1024 * 1024 * 4), G.empty(w * h)
    masks = np.empty((len(cands), h, w), np.uint8)
    for k, c in enumerate(cands):
        p, plane = divmod(int(c), 3)
        chosen = G.dev(np.array([plane], np.int32))
        L.vx_check(G.api().vx_sam_process_masks(src.ptr + p * 4 * n_px * 2, 4 * n_px, n_px, 1, 256, 4, chosen.ptr, scaled.ptr, 1024, sw, sh, out.ptr, w, h, 1, None))
        G.sync()
        masks[k] = out.to_numpy(np.uint8, (h, w))
    return masks


def _assert_equals_reference(run, thresholds, max_masks, w, h, what):
    """everything the call returned against the reference on the call's own logits -> the reference's select() result"""
    pt, st, off, nt = thresholds
    sel = R.select(run["logits"], run["iou"], w, h, pred_iou_thresh=pt, stability_thresh=st, stability_offset=off, nms_iou_thresh=nt, capacity=max_masks)
    assert run["counts"] == sel["counts"], (what, run["counts"], sel["counts"])
    keep = sel["keep"]
    np.testing.assert_array_equal(run["info_i32"][:, 0] * 3 + run["info_i32"][:, 1], keep, err_msg=what)
    want_masks = _masks_by_process_masks(run["logits"], keep, w, h)
    assert run["masks"].tobytes() == want_masks.tobytes(), what
    want_i = np.array([[c // 3, c % 3, *R.mask_stats(want_masks[k]), 0] for k, c in enumerate(keep)], np.int32).reshape(len(keep), 8)
    np.testing.assert_array_equal(run["info_i32"], want_i, err_msg=what)
    assert run["info_f32"][:, 0].tobytes() == sel["cand_iou"][keep].tobytes(), what
    stab = sel["stability"][keep]
    assert (np.abs(run["info_f32"][:, 1].astype(np.float64) - stab) <= np.spacing(np.abs(stab))).all(), (what, run["info_f32"][:, 1], stab)
    return sel


@pytest.fixture(scope="module")
def sam(tmp_path_factory):
    from visioncpp_amd import synth, vision
    tmp = tmp_path_factory.mktemp("samautogen")
    cfg = synth.TINYVIT_5M
    path = synth.write_mobile_sam_gguf(tmp / "mobile_sam.gguf", cfg, enc_sd=synth.tinyvit_state_dict(cfg, R.SCENARIO_ENCODER_SEED), dec_sd=R.scenario_decoder_state_dict())
    dev = vision.Device.init(vision.Backend.gpu)
    model = vision.Model.load(path, dev)
    model.enable_captures(True)
    s = dict(model=model, dev=dev, path=path, encoded=None, prompts=R.scenario_prompts())
    _encode31(s)
    yield s
    s.pop("model")
    s.pop("dev")


@pytest.fixture(scope="module")
def scenario(sam):
    """the thresholds, from the values a first call captured, and the call at those thresholds"""
    _encode31(sam)
    from visioncpp_amd import vision
    dflt = vision.sam_generate_defaults()
    first = _generate(sam, sam["prompts"], (dflt["pred_iou_thresh"], dflt["stability_thresh"], dflt["stability_offset"], dflt["nms_iou_thresh"]), 64)
    picked = R.pick_thresholds((first["logits"], first["iou"]), 1024, 1024, stability_offset=1.0)
    assert picked is not None, "the captured values admit no thresholds with the four conditions"
    thresholds = (picked[0], picked[1], 1.0, picked[2])
    run = _generate(sam, sam["prompts"], thresholds, 64)
    assert run["logits"].tobytes() == first["logits"].tobytes() and run["iou"].tobytes() == first["iou"].tobytes(), "the same decode twice gave other bytes"
    return dict(first=first, thresholds=thresholds, run=run)


def test_generate_equals_the_reference_on_its_own_logits(sam, scenario):
    run, thresholds = scenario["run"], scenario["thresholds"]
    assert run["logits"].shape == (18, 4, 256, 256) and run["iou"].shape == (18, 4)
    sel = R.select(run["logits"], run["iou"], 1024, 1024, pred_iou_thresh=thresholds[0], stability_thresh=thresholds[1], stability_offset=thresholds[2],
                   nms_iou_thresh=thresholds[3], capacity=64)
    c = R.scenario_conditions(sel, thresholds[0])
    print(f"thresholds {thresholds}: {c}")
    R.assert_scenario(c)  # conditions on the reference, before anything is compared
    _assert_equals_reference(run, thresholds, 64, 1024, 1024, "scenario")
    assert run["masks"].shape == (c["kept"], 1024, 1024) and set(np.unique(run["masks"])) <= {0, 255}
    # SAM's defaults on the same decode (whatever they keep)
    dflt = (0.88, 0.95, 1.0, 0.7)
    _assert_equals_reference(scenario["first"], tuple(np.float32(v) for v in dflt), 64, 1024, 1024, "defaults")
    again = _generate(sam, sam["prompts"], thresholds, 64)
    for k in ("masks", "info_i32", "info_f32", "logits", "iou"):
        assert again[k].tobytes() == run[k].tobytes(), f"the same call twice gave other {k}"


def test_logits_and_chosen_masks_are_the_batch_calls(sam, scenario):
    m = sam["model"]
    _encode31(sam)
    m.sam_set_prompt_chunk(CHUNK)
    masks, iou, chosen = m.sam_compute_batch(sam["prompts"])
    logits, iou2 = m.sam_read_masks_batch()
    run = scenario["run"]
    assert logits.astype(np.float16).tobytes() == run["logits"].tobytes(), "the logits of the generate call are not the batch call's"
    assert iou.tobytes() == run["iou"].tobytes() == iou2.tobytes()
    same_plane = 0
    for k, row in enumerate(run["info_i32"]):
        if chosen[row[0]] == row[1]:
            same_plane += 1
            assert run["masks"][k].tobytes() == masks[row[0]].tobytes(), f"kept mask {k} (prompt {row[0]}, plane {row[1]})"
    print(f"{same_plane} of {len(run['info_i32'])} kept masks are their prompt's chosen plane")


def test_other_calls_keep_their_bytes_across_a_generate_call(sam, scenario):
    m = sam["model"]
    _encode31(sam)
    m.sam_set_prompt_chunk(CHUNK)
    some = [sam["prompts"][5], sam["prompts"][16]]

    def others():
        out = []
        for p in some:
            mask = m.sam_compute(p)
            logits, iou = m.sam_read_masks()
            out += [mask, logits, iou]
        out += list(m.sam_compute_batch(sam["prompts"][:5]))
        out += list(m.sam_read_masks_batch())
        return out

    before = others()
    _generate(sam, sam["prompts"], scenario["thresholds"], 64)
    after = others()
    for b, a in zip(before, after):
        assert b.tobytes() == a.tobytes(), "a call changed across a generate call"


def test_capacity_cuts_the_list(sam, scenario):
    _encode31(sam)
    full = scenario["run"]
    assert full["counts"][1] >= 2  # the scenario keeps at least two: capacity 1 cuts
    for cap in (1, 2):
        cut = _generate(sam, sam["prompts"], scenario["thresholds"], cap)
        assert cut["counts"] == (cap, full["counts"][1])
        for k in ("masks", "info_i32", "info_f32"):
            assert cut[k].tobytes() == full[k][:cap].tobytes(), (cap, k)
        _assert_equals_reference(cut, scenario["thresholds"], cap, 1024, 1024, f"capacity {cap}")


def test_python_records_and_other_chunks(sam, scenario):
    m = sam["model"]
    _encode31(sam)
    run, (pt, st, off, nt) = scenario["run"], scenario["thresholds"]
    m.sam_set_prompt_chunk(CHUNK)
    recs = m.sam_generate_masks(prompts=sam["prompts"], pred_iou_thresh=pt, stability_thresh=st, stability_offset=off, nms_iou_thresh=nt, max_masks=64)
    assert len(recs) == run["counts"][0]
    for k, r in enumerate(recs):
        row = run["info_i32"][k]
        assert r["segmentation"].dtype == bool and np.array_equal(r["segmentation"], run["masks"][k] == 255)
        assert r["area"] == row[6] == int(r["segmentation"].sum()) and r["bbox"] == [int(v) for v in row[2:6]]
        assert r["predicted_iou"] == run["info_f32"][k, 0] and r["stability_score"] == run["info_f32"][k, 1]
        prompt = sam["prompts"][row[0]]
        assert (r["point_coords"] == [prompt] and "box" not in r) if len(prompt) == 2 else (r["box"] == prompt and "point_coords" not in r)
    assert [r["predicted_iou"] for r in recs] == sorted((r["predicted_iou"] for r in recs), reverse=True)
    # another chunking (one chunk of 18): other sums in layer 0, so other logits -- and the call still equals the reference on ITS logits
    whole = _generate(sam, sam["prompts"], scenario["thresholds"], 64, chunk=64)
    _assert_equals_reference(whole, scenario["thresholds"], 64, 1024, 1024, "chunk 64")


def test_non_square_image_host_and_device_entries_agree(sam):
    from tests import gpu_util as G
    from visioncpp_amd import synth
    m = sam["model"]
    m.sam_encode(synth.images(1, 640, 480, seed=8)[0])
    sam["encoded"] = None
    assert m.sam_image_extent() == (640, 480)
    prompts = R.scenario_prompts(640, 480)[:16:3] + [[100, 80, 500, 400]]
    first = _generate(sam, prompts, (-np.inf, -np.inf, 1.0, 1.0), 32, chunk=4)
    picked = R.pick_thresholds((first["logits"], first["iou"]), 640, 480)
    thresholds = (picked[0], picked[1], 1.0, picked[2]) if picked else (float(np.median(first["iou"][:, :3])), 0.0, 1.0, 0.9)
    cap = 8
    host = _generate(sam, prompts, thresholds, cap, chunk=4)
    sel = _assert_equals_reference(host, thresholds, cap, 640, 480, "640x480 host")
    assert host["masks"].shape[1:] == (480, 640) and sel["counts"][0] >= 1
    px, GUARDED = 640 * 480, 64
    dm, di = G.dev(np.full(cap * px + GUARDED, 7, np.uint8)), G.dev(np.full(cap * 8 + GUARDED, -7, np.int32))
    df, dc = G.dev(np.full(cap * 2 + GUARDED, -7.0, np.float32)), G.dev(np.full(2 + GUARDED, -7, np.int32))
    m.sam_generate_masks_device(prompts, dm.ptr, di.ptr, df.ptr, dc.ptr, max_masks=cap, pred_iou_thresh=thresholds[0], stability_thresh=thresholds[1],
                                stability_offset=thresholds[2], nms_iou_thresh=thresholds[3])
    G.sync()
    r = host["counts"][0]
    counts = dc.to_numpy(np.int32, (2 + GUARDED,))
    assert tuple(counts[:2]) == host["counts"] and (counts[2:] == -7).all()
    gm, gi, gf = dm.to_numpy(np.uint8, (cap * px + GUARDED,)), di.to_numpy(np.int32, (cap * 8 + GUARDED,)), df.to_numpy(np.float32, (cap * 2 + GUARDED,))
    assert gm[: r * px].tobytes() == host["masks"].tobytes() and (gm[r * px:] == 7).all(), "masks: the device entry differs, or wrote behind the returned masks"
    assert gi[: r * 8].tobytes() == host["info_i32"].tobytes() and (gi[r * 8:] == -7).all()
    assert gf[: r * 2].tobytes() == host["info_f32"].tobytes() and (gf[r * 2:] == -7.0).all()


def test_errors(sam, tmp_path):
    from visioncpp_amd import _lib as L, synth, vision
    m = sam["model"]
    _encode31(sam)
    fresh = vision.Model.load(synth.write_mobile_sam_gguf(tmp_path / "s.gguf", seed=4), m._device)
    with pytest.raises(L.Error, match="call sam_encode"):
        fresh.sam_generate_masks_raw([[1, 2]])
    with pytest.raises(L.Error, match="call sam_encode"):
        fresh.sam_generate_masks_device([[1, 2]], 4096, 4096, 4096, 4096)
    with pytest.raises(L.Error, match="must be 2 or 4"):
        m.sam_generate_masks_raw([[1, 2], [1, 2, 3]])
    with pytest.raises(L.Error, match="empty batch"):
        m.sam_generate_masks_raw([])
    with pytest.raises(L.Error, match="at most 5461"):
        m.sam_generate_masks_raw([[1, 2]] * 5462, max_masks=1)
    with pytest.raises(L.Error, match="NaN"):
        m.sam_generate_masks_raw([[1, 2]], pred_iou_thresh=float("nan"))
    with pytest.raises(L.Error, match=r"outside \[0, 1\]"):
        m.sam_generate_masks_raw([[1, 2]], nms_iou_thresh=1.5)
    with pytest.raises(L.Error, match="below 0"):
        m.sam_generate_masks_raw([[1, 2]], stability_offset=-1.0)
    with pytest.raises(L.Error, match="capacity"):
        m.sam_generate_masks_raw([[1, 2]], max_masks=0)
    api = L.get_lib()
    p, k = vision.Model._sam_prompt_arrays([[1, 2]])
    for outs in ((None, 4096, 4096, 4096), (4096, None, 4096, 4096), (4096, 4096, None, 4096), (4096, 4096, 4096, None)):
        assert api.visp_sam_generate_masks_device(m._handle, p.ctypes.data, k.ctypes.data, 1, 0.88, 0.95, 1.0, 0.7, 4, *outs, None) == 0
        assert b"null" in api.visp_get_last_error()
        assert api.visp_sam_generate_masks_host(m._handle, p.ctypes.data, k.ctypes.data, 1, 0.88, 0.95, 1.0, 0.7, 4, *outs) == 0
        assert b"null" in api.visp_get_last_error()
    enc_only = vision.Model.load(synth.write_tinyvit_gguf(tmp_path / "t.gguf", synth.TINYVIT_5M, seed=1), m._device)
    enc_only.sam_encode(synth.images(1, 64, 48, seed=3)[0])
    with pytest.raises(L.Error, match="dec"):
        enc_only.sam_generate_masks_raw([[1, 2]])
    m.enable_captures(False)
    try:
        m.sam_generate_masks_raw([[700, 300]], max_masks=2)
        with pytest.raises(L.Error, match="enable captures"):
            m.sam_read_masks_batch()
    finally:
        m.enable_captures(True)


def test_cpp_overloads_of_vision_h(sam):
    """tests/cpp/sam_autogen_check.cpp: sam_point_grid and the sam_generate_masks overloads of include/visp/vision.h, each record held to its own mask, in a
    process of its own"""
    exe = Path(__file__).resolve().parents[1] / "vision.cpp_amd" / "lib" / "sam_autogen_check"
    assert exe.exists(), "build() makes it"
    r = subprocess.run([str(exe), str(sam["path"]), "320", "240"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    words = r.stdout.split()
    assert words[4:] == ["masks", "320x240", "ok"], r.stdout
    n_point, n_box, n_grid, n_cut = (int(v) for v in words[:4])
    assert 1 <= n_point <= 27 and 1 <= n_box <= 6 and n_grid == n_point and n_cut == min(2, n_point), r.stdout

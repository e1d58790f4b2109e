"""The min_region_area path of automatic mask generation (visp_sam_generate_masks_clean_* / Model.sam_generate_masks*(min_mask_region_area=...)) and the
primitive behind it (visp_image_remove_small_regions_*), on the scenario of tests/test_gpu_sam_autogen.py: the synthetic full-size model with the decoder of
tests/sam_select_ref.scenario_decoder_state_dict, the seed-31 image, the 4 x 4 grid plus two boxes at chunk 8.

With min_region_area 0 the new entries must return the bytes of the existing ones. With a min_region_area above 0, everything a call returns must EQUAL
tests/sam_regions_ref.postprocess applied to the call's OWN first stage: the output of the same call with min_region_area 0, whose decode is asserted to be the
same bytes through the captured logits. The scenario runs with the filters open and the NMS threshold picked from its own values as test_gpu_sam_autogen.py
picks it; its min_region_area is picked from its own first-stage masks (sam_regions_ref.pick_min_region_area) so that some masks change, some do not and the
second NMS removes at least one: asserted here before anything is compared. tests/test_sam_regions_ref_cpu.py shows with the oracle that such a value exists."""
import subprocess
import time
from pathlib import Path

import numpy as np
import pytest

from tests import sam_regions_ref as RR
from tests import sam_select_ref as R

pytestmark = pytest.mark.gpu

CHUNK = 8
INF = float("inf")


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


def _generate(s, prompts, thresholds, max_masks, area, chunk=CHUNK):
    """one host call with captures -> dict(masks, info_i32, info_f32, counts, logits f16, iou)"""
    m = s["model"]
    m.sam_set_prompt_chunk(chunk)
    pt, st, off, nt = thresholds
    masks, ii, fi, counts = m.sam_generate_masks_raw(prompts, pred_iou_thresh=pt, stability_thresh=st, stability_offset=off, nms_iou_thresh=nt, max_masks=max_masks,
                                                     min_mask_region_area=area)
    logits, iou = m.sam_read_masks_batch()
    return dict(masks=masks, info_i32=ii, info_f32=fi, counts=counts, logits=logits.astype(np.float16), iou=iou)


def _assert_equals_reference(run, first, area, nt, what):
    """a cleaning call against the reference on the first stage `first` (the same call with min_region_area 0) -> the reference's postprocess() result"""
    assert run["logits"].tobytes() == first["logits"].tobytes() and run["iou"].tobytes() == first["iou"].tobytes(), f"{what}: the decode differs from the first stage's"
    post = RR.postprocess(first["masks"], first["info_i32"], first["info_f32"], area, nt)
    assert run["counts"] == (len(post["keep"]), first["counts"][1], post["changed_count"], post["removed"]), (what, run["counts"], post["keep"], post["changed"])
    assert run["masks"].tobytes() == post["masks"].tobytes(), f"{what}: masks"
    np.testing.assert_array_equal(run["info_i32"], post["info_i32"], err_msg=what)
    assert run["info_f32"].tobytes() == post["info_f32"].tobytes(), f"{what}: info_f32"
    return post


@pytest.fixture(scope="module")
def sam(tmp_path_factory):
    from visioncpp_amd import synth, vision
    tmp = tmp_path_factory.mktemp("samregions")
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
    """the thresholds and the min_region_area, from the values the call itself produced, and the first stage at those thresholds"""
    _encode31(sam)
    probe = _generate(sam, sam["prompts"], (-INF, -INF, 1.0, 1.0), 64, 0)
    picked = R.pick_thresholds((probe["logits"], probe["iou"]), 1024, 1024, stability_offset=1.0)
    assert picked is not None, "the captured values admit no thresholds with the four conditions"
    thresholds = (-INF, -INF, 1.0, picked[2])
    first = _generate(sam, sam["prompts"], thresholds, 64, 0)
    area = RR.pick_min_region_area(first["masks"], first["info_i32"], first["info_f32"], thresholds[3])
    assert area is not None, "the first-stage masks admit no min_region_area with the three conditions"
    return dict(thresholds=thresholds, first=first, area=area)


def test_min_region_area_0_returns_the_bytes_of_the_existing_entries(sam, scenario):
    from tests import gpu_util as G
    from visioncpp_amd import _lib as L, vision
    m, first, (pt, st, off, nt) = sam["model"], scenario["first"], scenario["thresholds"]
    _encode31(sam)
    m.sam_set_prompt_chunk(CHUNK)
    api = L.get_lib()
    p, k = vision.Model._sam_prompt_arrays(sam["prompts"])
    cap, px, r = 64, 1024 * 1024, first["counts"][0]
    masks, ii, fi, counts = np.full((cap, 1024, 1024), 7, np.uint8), np.full((cap, 8), -7, np.int32), np.full((cap, 2), -7, np.float32), np.full(4, -7, np.int32)
    L.check(api.visp_sam_generate_masks_clean_host(m._handle, p.ctypes.data, k.ctypes.data, len(k), pt, st, off, nt, cap, 0, masks.ctypes.data, ii.ctypes.data, fi.ctypes.data,
                                                   counts.ctypes.data))
    assert tuple(counts[:2]) == first["counts"] and (counts[2:] == -7).all()
    assert masks[:r].tobytes() == first["masks"].tobytes() and (masks[r:] == 7).all()
    assert ii[:r].tobytes() == first["info_i32"].tobytes() and (ii[r:] == -7).all() and fi[:r].tobytes() == first["info_f32"].tobytes() and (fi[r:] == -7).all()
    GUARD = 64
    dm, di = G.dev(np.full(cap * px + GUARD, 7, np.uint8)), G.dev(np.full(cap * 8 + GUARD, -7, np.int32))
    df, dc = G.dev(np.full(cap * 2 + GUARD, -7.0, np.float32)), G.dev(np.full(4 + GUARD, -7, np.int32))
    L.check(api.visp_sam_generate_masks_clean_device(m._handle, p.ctypes.data, k.ctypes.data, len(k), pt, st, off, nt, cap, 0, dm.ptr, di.ptr, df.ptr, dc.ptr, None))
    G.sync()
    c = dc.to_numpy(np.int32, (4 + GUARD,))
    assert tuple(c[:2]) == first["counts"] and (c[2:] == -7).all()
    gm = dm.to_numpy(np.uint8, (cap * px + GUARD,))
    assert gm[: r * px].tobytes() == first["masks"].tobytes() and (gm[r * px:] == 7).all()
    assert di.to_numpy(np.int32, (cap * 8 + GUARD,))[: r * 8].tobytes() == first["info_i32"].tobytes()
    assert df.to_numpy(np.float32, (cap * 2 + GUARD,))[: r * 2].tobytes() == first["info_f32"].tobytes()


def test_cleaning_equals_the_reference_on_its_own_first_stage(sam, scenario):
    _encode31(sam)
    first, area, thresholds = scenario["first"], scenario["area"], scenario["thresholds"]
    post = RR.postprocess(first["masks"], first["info_i32"], first["info_f32"], area, thresholds[3])
    c = RR.scenario_conditions(post, len(first["masks"]))
    print(f"thresholds {thresholds}, {len(first['masks'])} first-stage masks, min_region_area {area}: {c}")
    RR.assert_scenario(c)  # conditions on the reference, before anything is compared
    run = _generate(sam, sam["prompts"], thresholds, 64, area)
    _assert_equals_reference(run, first, area, thresholds[3], "scenario")
    flags = run["info_i32"][:, 7]
    assert (np.diff(flags) >= 0).all() and all((np.diff(run["info_f32"][flags == f, 0]) <= 0).all() for f in (0, 1))  # SAM's order
    again = _generate(sam, sam["prompts"], thresholds, 64, area)
    for key in ("masks", "info_i32", "info_f32", "logits", "iou"):
        assert again[key].tobytes() == run[key].tobytes(), f"the same call twice gave other {key}"
    assert again["counts"] == run["counts"]
    # other values on the same first stage: speckle-sized ones, at which the second NMS may remove nobody
    for other in (2, 40):
        _assert_equals_reference(_generate(sam, sam["prompts"], thresholds, 64, other), first, other, thresholds[3], f"min_region_area {other}")
    # the records of the Python layer stay SAM's dicts
    m = sam["model"]
    recs = m.sam_generate_masks(prompts=sam["prompts"], pred_iou_thresh=thresholds[0], stability_thresh=thresholds[1], stability_offset=thresholds[2],
                                nms_iou_thresh=thresholds[3], max_masks=64, min_mask_region_area=area)
    assert len(recs) == run["counts"][0]
    for r, mask, row in zip(recs, run["masks"], run["info_i32"]):
        assert np.array_equal(r["segmentation"], mask == 255) and r["area"] == row[6] and r["bbox"] == [int(v) for v in row[2:6]]
        assert set(r) <= {"segmentation", "area", "bbox", "predicted_iou", "stability_score", "point_coords", "box"}


def test_capacity_1(sam, scenario):
    """the first stage cut to one mask, which is then cleaned: the reference on that one-mask first stage"""
    _encode31(sam)
    first, area, thresholds = scenario["first"], scenario["area"], scenario["thresholds"]
    assert first["counts"][1] >= 2
    one = _generate(sam, sam["prompts"], thresholds, 1, 0)
    assert one["counts"] == (1, first["counts"][1]) and one["masks"].tobytes() == first["masks"][:1].tobytes()
    for a in (area, 2):
        cut = _generate(sam, sam["prompts"], thresholds, 1, a)
        post = _assert_equals_reference(cut, one, a, thresholds[3], f"capacity 1, min_region_area {a}")
        assert len(post["keep"]) == 1


def test_other_calls_keep_their_bytes_across_a_cleaning_call(sam, scenario):
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
        plain = _generate(sam, sam["prompts"], scenario["thresholds"], 64, 0)
        out += [plain["masks"], plain["info_i32"], plain["info_f32"]]
        return out

    before = others()
    _generate(sam, sam["prompts"], scenario["thresholds"], 64, scenario["area"])
    after = others()
    for b, a in zip(before, after):
        assert b.tobytes() == a.tobytes(), "a call changed across a cleaning call"


def test_the_primitive_on_the_masks_of_a_batch_call(sam):
    """visp_image_remove_small_regions_* on the masks of sam_compute_batch: the reference's bytes, and the bytes of the launcher as tests/test_gpu_regions_kernels.py
    calls it; device and host entries, each mode"""
    from tests import gpu_util as G
    from visioncpp_amd import _lib as L, vision
    m = sam["model"]
    _encode31(sam)
    m.sam_set_prompt_chunk(CHUNK)
    masks, _, _ = m.sam_compute_batch(sam["prompts"][:6])
    n, h, w = masks.shape
    assert (h, w) == (1024, 1024) and masks.any()
    api = L.get_lib()
    for mode_name, mode in (("both", RR.BOTH), ("holes", RR.HOLES), ("islands", RR.ISLANDS)):
        want, want_changed = RR.remove_small_regions(masks, 30, mode)
        got, changed = vision.remove_small_regions(masks, 30, mode_name, device=sam["dev"])
        assert got.tobytes() == want.tobytes() and changed.tolist() == want_changed.astype(bool).tolist(), mode_name
        md, cd = G.dev(masks), G.dev(np.full(n, -7, np.int32))
        vision.remove_small_regions_device(md.ptr, n, w, h, 30, mode_name, cd.ptr, device=sam["dev"])
        assert md.to_numpy(np.uint8, (n, h, w)).tobytes() == want.tobytes() and cd.to_numpy(np.int32, (n,)).tolist() == want_changed.tolist(), mode_name
        kd, kc = G.dev(masks), G.dev(np.full(n, -7, np.int32))
        ws_bytes = api.vx_mask_regions_workspace_bytes(w, h, 2)
        ws = G.empty(ws_bytes)
        L.vx_check(api.vx_mask_remove_small_regions_u8(kd.ptr, w, h, n, None, 30, mode, kc.ptr, ws.ptr, ws_bytes, 2, None))
        G.sync()
        assert kd.to_numpy(np.uint8, (n, h, w)).tobytes() == want.tobytes() and kc.to_numpy(np.int32, (n,)).tolist() == want_changed.tolist(), mode_name
    one, flag = vision.remove_small_regions(masks[0], 30)
    assert one.shape == (h, w) and one.tobytes() == RR.remove_small_regions(masks[0], 30)[0].tobytes() and isinstance(flag, bool)
    with pytest.raises(L.Error, match="min_area"):
        vision.remove_small_regions(masks[:1], -1)


def test_the_glue_kernels_of_the_second_nms():
    """vx_sam_clean_nms_inputs and vx_sam_gather_clean_masks on hand-made rows: an unaligned extent, a count below the rows, an index list that reorders"""
    from tests import gpu_util as G
    from visioncpp_amd import _lib as L
    api = L.get_lib()
    L.vx_check(api.vx_set_device(0))
    rng = np.random.default_rng(3)
    N, w, h, live = 6, 13, 7, 5
    masks = np.where(rng.random((N, h, w)) < 0.5, 255, 0).astype(np.uint8)
    masks[2] = 0
    info = np.zeros((N, 8), np.int32)
    for i in range(N):
        info[i] = [i, i % 3, *R.mask_stats(masks[i]), 0]
    info_f = rng.random((N, 2)).astype(np.float32)
    changed = np.array([0, 1, 0, 1, 1, 0], np.int32)
    first = np.array([live, 9], np.int32)
    GUARD = 16
    table, key = G.dev(np.full(N * 6 + GUARD, -7, np.int32)), G.dev(np.full(N + GUARD, -7.0, np.float32))
    L.vx_check(api.vx_sam_clean_nms_inputs(G.dev(info).ptr, G.dev(changed).ptr, G.dev(first).ptr, N, table.ptr, key.ptr, None))
    G.sync()
    t, kk = table.to_numpy(np.int32, (N * 6 + GUARD,)), key.to_numpy(np.float32, (N + GUARD,))
    want_t = np.array([[1, 1, *RR.inclusive_box(masks[i])] if i < live else [1, 1, 0, 0, 0, 0] for i in range(N)], np.int32)
    assert t[: N * 6].reshape(N, 6).tolist() == want_t.tolist() and (t[N * 6:] == -7).all()
    assert kk[:live].tolist() == [1.0, 0.0, 1.0, 0.0, 0.0] and np.isnan(kk[live]) and (kk[N:] == -7.0).all()
    keep, second = np.array([2, 0, 4, 1, 7, 7], np.int32), np.array([4, 4], np.int32)
    px = w * h
    om, oi = G.dev(np.full(1 + N * px + GUARD, 7, np.uint8)), G.dev(np.full(N * 8 + GUARD, -7, np.int32))
    of, oc = G.dev(np.full(N * 2 + GUARD, -7.0, np.float32)), G.dev(np.full(4 + GUARD, -7, np.int32))
    L.vx_check(api.vx_sam_gather_clean_masks(G.dev(masks).ptr, w, h, G.dev(info).ptr, G.dev(info_f).ptr, G.dev(changed).ptr, G.dev(keep).ptr, G.dev(first).ptr,
                                             G.dev(second).ptr, N, om.ptr + 1, oi.ptr, of.ptr, oc.ptr, None))
    G.sync()
    gm, gi, gf, gc = om.to_numpy(np.uint8, (1 + N * px + GUARD,)), oi.to_numpy(np.int32, (N * 8 + GUARD,)), of.to_numpy(np.float32, (N * 2 + GUARD,)), oc.to_numpy(np.int32, (4 + GUARD,))
    assert gm[0] == 7 and gm[1: 1 + 4 * px].tobytes() == masks[keep[:4]].tobytes() and (gm[1 + 4 * px:] == 7).all()
    want_i = info[keep[:4]].copy()
    want_i[:, 7] = changed[keep[:4]]
    assert gi[: 32].reshape(4, 8).tolist() == want_i.tolist() and (gi[32:] == -7).all()
    assert gf[: 8].tobytes() == info_f[keep[:4]].tobytes() and (gf[8:] == -7.0).all()
    assert gc[:4].tolist() == [4, 9, 2, 1] and (gc[4:] == -7).all()
    for args in ((None, w, h, 1, 1, 1, 1, 1, 1, N, 1, 1, 1, 1, None), (1, 0, h, 1, 1, 1, 1, 1, 1, N, 1, 1, 1, 1, None), (1, w, h, 1, 1, 1, 1, 1, 1, 0, 1, 1, 1, 1, None)):
        with pytest.raises(L.Error, match="vx_sam_gather_clean_masks"):
            L.vx_check(api.vx_sam_gather_clean_masks(*args))
    for args in ((None, 1, 1, N, 1, 1, None), (1, 1, 1, 0, 1, 1, None)):
        with pytest.raises(L.Error, match="vx_sam_clean_nms_inputs"):
            L.vx_check(api.vx_sam_clean_nms_inputs(*args))


def test_non_square_image_host_and_device_entries_agree(sam):
    from tests import gpu_util as G
    from visioncpp_amd import synth
    m = sam["model"]
    m.sam_encode(synth.images(1, 640, 480, seed=8)[0])
    sam["encoded"] = None
    prompts = R.scenario_prompts(640, 480)[:16:3] + [[100, 80, 500, 400]]
    thresholds, cap = (-INF, -INF, 1.0, 0.9), 8
    first = _generate(sam, prompts, thresholds, cap, 0, chunk=4)
    assert first["masks"].shape[1:] == (480, 640) and first["counts"][0] >= 1
    area = RR.pick_min_region_area(first["masks"], first["info_i32"], first["info_f32"], thresholds[3]) or 40
    host = _generate(sam, prompts, thresholds, cap, area, chunk=4)
    _assert_equals_reference(host, first, area, thresholds[3], "640x480 host")
    px, GUARD = 640 * 480, 64
    dm, di = G.dev(np.full(cap * px + GUARD, 7, np.uint8)), G.dev(np.full(cap * 8 + GUARD, -7, np.int32))
    df, dc = G.dev(np.full(cap * 2 + GUARD, -7.0, np.float32)), G.dev(np.full(4 + GUARD, -7, np.int32))
    m.sam_generate_masks_device(prompts, dm.ptr, di.ptr, df.ptr, dc.ptr, max_masks=cap, pred_iou_thresh=thresholds[0], stability_thresh=thresholds[1],
                                stability_offset=thresholds[2], nms_iou_thresh=thresholds[3], min_mask_region_area=area)
    G.sync()
    r = host["counts"][0]
    counts = dc.to_numpy(np.int32, (4 + GUARD,))
    assert tuple(counts[:4]) == host["counts"] and (counts[4:] == -7).all()
    gm, gi, gf = dm.to_numpy(np.uint8, (cap * px + GUARD,)), di.to_numpy(np.int32, (cap * 8 + GUARD,)), df.to_numpy(np.float32, (cap * 2 + GUARD,))
    assert gm[: r * px].tobytes() == host["masks"].tobytes() and (gm[r * px:] == 7).all(), "masks: the device entry differs, or wrote behind the returned masks"
    assert gi[: r * 8].tobytes() == host["info_i32"].tobytes() and (gi[r * 8:] == -7).all()
    assert gf[: r * 2].tobytes() == host["info_f32"].tobytes() and (gf[r * 2:] == -7.0).all()


def test_errors_and_the_split(sam):
    from visioncpp_amd import _lib as L
    m = sam["model"]
    _encode31(sam)
    with pytest.raises(L.Error, match="min_region_area"):
        m.sam_generate_masks_raw([[1, 2]], min_mask_region_area=-3)
    m.sam_set_prompt_chunk(CHUNK)  # the 18 scenario prompts make three chunks: decode and scoring close three intervals each
    stages = ("decode_ms", "scoring_ms", "rank_nms_ms", "output_ms", "clean_ms", "records_nms2_ms", "gather_ms")
    m.enable_timing(True)
    try:
        t0 = time.perf_counter()
        m.sam_generate_masks_raw(sam["prompts"], pred_iou_thresh=-INF, stability_thresh=-INF, nms_iou_thresh=1.0, max_masks=8, min_mask_region_area=20)
        wall_ms = (time.perf_counter() - t0) * 1e3
        five = m.sam_generate_last_split5()
        four = m.sam_generate_last_split()
        assert all(five[k] == four[k] for k in four) and all(five[k] > 0 for k in stages), five
        assert abs(five["cleaning_ms"] - (five["clean_ms"] + five["records_nms2_ms"] + five["gather_ms"])) < 1e-3
        # the host call ends synchronised, so its intervals on the device lie inside it: a sum above the wall clock counted an interval twice
        assert sum(five[k] for k in stages) <= wall_ms, (five, wall_ms)
        m.sam_generate_masks_raw(sam["prompts"], pred_iou_thresh=-INF, stability_thresh=-INF, nms_iou_thresh=1.0, max_masks=8)
        five = m.sam_generate_last_split5()
        assert five["cleaning_ms"] == 0.0 and five["clean_ms"] == five["records_nms2_ms"] == five["gather_ms"] == 0.0, five
    finally:
        m.enable_timing(False)


def test_cpp_names_of_vision_h(sam):
    """tests/cpp/sam_regions_check.cpp: image_remove_small_regions, sam_generate_params::min_mask_region_area and sam_mask::cleaned, in a process of its own"""
    exe = Path(__file__).resolve().parents[1] / "vision.cpp_amd" / "lib" / "sam_regions_check"
    assert exe.exists(), "build() makes it"
    r = subprocess.run([str(exe), str(sam["path"]), "320", "240"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    words = r.stdout.split()
    assert words[3:] == ["masks", "320x240", "ok"], r.stdout
    n_plain, n_clean, n_changed = (int(v) for v in words[:3])
    assert 1 <= n_plain <= 27 and n_clean == n_plain and n_changed <= n_clean, r.stdout

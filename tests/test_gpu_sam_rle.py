"""Model.sam_generate_masks(output_mode="uncompressed_rle") on the scenario of tests/test_gpu_sam_regions.py (the synthetic full-size model with the decoder of
tests/sam_select_ref.scenario_decoder_state_dict, the seed-31 image, the 4 x 4 grid plus two boxes): record for record, the segmentation is tests/rle_ref.py of
the segmentation that output_mode="binary_mask" returns on the same arguments, and every other key is equal."""
import numpy as np
import pytest

from tests import rle_ref as RR
from tests import sam_select_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    from visioncpp_amd import synth, vision
    cfg = synth.TINYVIT_5M
    path = synth.write_mobile_sam_gguf(tmp_path_factory.mktemp("samrle") / "mobile_sam.gguf", cfg, enc_sd=synth.tinyvit_state_dict(cfg, R.SCENARIO_ENCODER_SEED),
                                       dec_sd=R.scenario_decoder_state_dict())
    dev = vision.Device.init(vision.Backend.gpu)
    m = vision.Model.load(path, dev)
    m.sam_set_prompt_chunk(8)
    m.sam_encode(synth.images(1, 320, 240, seed=R.SCENARIO_IMAGE_SEED)[0])
    yield m
    del m, dev


@pytest.mark.parametrize("area", [0, 40])
def test_rle_records_equal_the_reference_of_the_binary_records(model, area):
    kw = dict(prompts=R.scenario_prompts(320, 240), pred_iou_thresh=-float("inf"), stability_thresh=-float("inf"), nms_iou_thresh=0.9, max_masks=12,
              min_mask_region_area=area)
    binary = model.sam_generate_masks(output_mode="binary_mask", **kw)
    rle = model.sam_generate_masks(output_mode="uncompressed_rle", **kw)
    assert len(rle) == len(binary) >= 2
    for b, r in zip(binary, rle):
        assert r["segmentation"] == RR.mask_to_rle(b["segmentation"])
        assert set(r) == set(b) and all(r[k] == b[k] for k in b if k != "segmentation")
    assert any(0 < len(r["segmentation"]["counts"]) - 1 for r in rle), "every mask is empty: the scenario shows nothing"

"""What visp_sam_predict_* decides without a device: the token rows per prompt shape (SAM's PromptEncoder.forward: k points, then one padding token or the
box's two corners, behind the iou token and the four mask tokens), the refusals that come before the model handle is looked at, and the reference of the
mask-input prompt (tests/sam_dense_ref.py) against torch's own Conv2d / GELU on the same weights."""
import ctypes as C

import numpy as np
import pytest

from tests import sam_dense_ref as R
from visioncpp_amd import _lib as L, synth


@pytest.mark.parametrize("k,box,want", [(1, 0, 7), (3, 0, 9), (0, 1, 7), (1, 1, 8), (64, 1, 71)])
def test_token_rows_per_prompt_shape(k, box, want):
    n = C.c_int32()
    L.check(L.get_lib().visp_sam_prompt_token_count(k, box, C.byref(n)))
    assert n.value == want


@pytest.mark.parametrize("k,box,labels,n,plane,message", [
    (1, False, [2], 1, -1, "label 2 of point 0 of prompt 0"), (2, True, [1, -2], 1, 0, "label -2 of point 1"), (0, False, [], 1, -1, "a point or a box"),
    (-1, True, [], 1, -1, "points per prompt"), (65, True, [1] * 65, 1, -1, "points per prompt"), (1, False, [1], 1, 4, "-1 .. 3"), (1, False, [1], 1, -2, "-1 .. 3"),
    (1, False, [1], 0, -1, "empty batch")])
def test_refusals_that_need_no_model(k, box, labels, n, plane, message):
    api = L.get_lib()
    pts, lab, bx, one = np.zeros((max(k, 1), 2), np.int32), np.array(labels + [0], np.int32), np.zeros(4, np.int32), np.ones(1, np.int32)
    for entry in (lambda: api.visp_sam_predict_host(None, pts.ctypes.data, lab.ctypes.data, k, bx.ctypes.data if box else None, None, 0, n, plane, None, None, None, None),
                  lambda: api.visp_sam_predict_device(None, pts.ctypes.data, lab.ctypes.data, k, bx.ctypes.data if box else None, None, 0, n, plane, None, None, None, None, None)):
        assert entry() == 0 and message.encode() in api.visp_get_last_error(), api.visp_get_last_error()
    assert api.visp_sam_predict_host(None, pts.ctypes.data, one.ctypes.data, 1, None, None, 0, 1, -1, None, None, None, None) == 0  # passes the checks, then has no model
    assert b"label" not in api.visp_get_last_error()
    count = C.c_int32()
    assert api.visp_sam_prompt_token_count(0, 0, C.byref(count)) == 0 and api.visp_sam_prompt_token_count(1, 0, None) == 0


def test_synthetic_mask_downscaling_leaves_every_other_tensor_alone_and_the_reference_is_torchs():
    import torch
    without, sd = synth.sam_decoder_state_dict(11), synth.sam_decoder_state_dict(11, mask_input=True)
    assert list(sd)[: len(without)] == list(without) and all(sd[k].tobytes() == v.tobytes() for k, v in without.items()) and len(sd) == len(without) + 10
    W = R.weights(sd)
    t = {k: torch.tensor(v) for k, v in W.items()}
    mask = np.random.default_rng(5).standard_normal((2, 20, 20)) * 5

    def norm(x, w, b):  # SAM's LayerNorm2d
        u = x.mean(1, keepdim=True)
        s = (x - u).pow(2).mean(1, keepdim=True)
        return w[:, None, None] * ((x - u) / torch.sqrt(s + R.EPS)) + b[:, None, None]

    F = torch.nn.functional
    x = F.gelu(norm(F.conv2d(torch.tensor(mask)[:, None], t["0.weight"], t["0.bias"], stride=2), t["1.weight"], t["1.bias"]))
    x = F.gelu(norm(F.conv2d(x, t["3.weight"], t["3.bias"], stride=2), t["4.weight"], t["4.bias"]))
    act, out = R.dense(mask, W)
    np.testing.assert_allclose(act, x.permute(0, 2, 3, 1).numpy(), atol=1e-3)  # ours is rounded to f16 here
    want = F.conv2d(torch.tensor(act).permute(0, 3, 1, 2), t["6.weight"], t["6.bias"]).permute(0, 2, 3, 1).numpy()
    np.testing.assert_allclose(out, want, rtol=0, atol=1e-12)

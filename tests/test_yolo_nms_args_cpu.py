"""What vx_yolo_nms refuses, it refuses with a message of its own before anything touches a device: these run without a GPU."""
import ctypes as C

import pytest

from visioncpp_amd import _lib as L

_buf = C.create_string_buffer(128)
P = (C.addressof(_buf) + 15) & ~15  # 16-byte aligned, never read: every call below is refused first
GOOD = dict(boxes=P, cand_count=P, cand_idx=P, cand_score=P, B=1, A=8, nc=3, iou=0.45, max_det=300, max_nms=100, max_wh=640, workspace=P, workspace_bytes=1 << 20,
            out=P, counts=P, stream=None)

BAD = [(dict(boxes=None), b"null operand"), (dict(counts=None), b"null operand"), (dict(boxes=P + 4), b"misaligned"), (dict(cand_idx=P + 2), b"misaligned"),
       (dict(out=P + 1), b"misaligned"), (dict(workspace=P + 8), b"workspace of"), (dict(B=0), b"batch 0"), (dict(A=0), b"0 anchors"), (dict(nc=0), b"x 0 classes"),
       (dict(max_det=0), b"max_det 0"), (dict(max_det=4097), b"max_det 4097"), (dict(max_nms=0), b"max_nms 0"), (dict(iou=-0.1), b"outside [0, 1]"),
       (dict(iou=1.5), b"outside [0, 1]"), (dict(iou=float("nan")), b"outside [0, 1]"), (dict(workspace_bytes=24 * 24 - 1), b"workspace of 575 bytes")]


@pytest.mark.parametrize("change, needle", BAD, ids=[f"{k}-{i}" for i, (c, _) in enumerate(BAD) for k in c])
def test_launcher_refuses_before_any_device_call(change, needle):
    api = L.get_lib()
    assert api.vx_yolo_nms(*{**GOOD, **change}.values()) == 0 and needle in api.vx_last_error(), api.vx_last_error()


def test_workspace_is_the_ranked_entries_of_every_image(ws=L.get_lib().vx_yolo_nms_workspace_bytes):
    # min(A nc, max_nms) rows of 16 + 8 bytes, 256-byte units; 0 for what the launcher refuses
    assert ws(1, 8, 3, 100) == ws(1, 8, 3, 24) == 512 + 256 and ws(4, 8, 3, 16) == 1024 + 512 and ws(1, 8, 3, 0) == 0 and ws(0, 8, 3, 10) == 0

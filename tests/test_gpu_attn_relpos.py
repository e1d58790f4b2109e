"""-m gpu: vx_attention_relpos_f16 (csrc/kernels_attn_relpos.hip) against the float64 reference and the derived per-element allowance of
tests/relpos_attn_ref.py. The output buffer starts zeroed and is compared in full, GUARD_ROWS zeroed rows behind the last row the call owns included (one
full query block): an element the call must not write has allowance 0 and must still hold zero bits. The same bits come out of a second call."""
import numpy as np
import pytest

import relpos_attn_ref as R
from buffer_check import assert_buffer
from visioncpp_amd import _lib as L

pytestmark = pytest.mark.gpu

from gpu_util import api, dev, empty, release, sync  # noqa: E402

GUARD_ROWS = 128  # the largest query block of the kernel


@pytest.fixture(autouse=True)
def _release_buffers():
    assert api().vx_device_count() > 0, "no HIP device visible: the product path has no CPU fallback"
    yield
    release()


def _launch(a, d, shape):
    out = empty(shape[0] * shape[1] * 2)
    L.vx_check(api().vx_attention_relpos_f16(d["q"].ptr, d["k"].ptr, d["v"].ptr, d["rel_h"].ptr, d["rel_w"].ptr, out.ptr, a["B"], a["H"], a["gw"], a["gh"], R.HD,
                                             float(a["scale"]), None))
    sync()
    return out.to_numpy(np.float16, shape)


@pytest.mark.parametrize("case", R.CASES, ids=[str(c) for c in R.CASES])
def test_attention_relpos_against_float64(case):
    a = R.operands(case)
    assert api().vx_attention_relpos_aligned(a["gw"], a["gh"]) == (1 if a["gw"] == 64 else 0)
    ref = R.evaluate_relpos(a, GUARD_ROWS)
    d = {name: dev(a[name]) for name in ("q", "k", "v", "rel_h", "rel_w")}
    got = _launch(a, d, ref[0].shape)
    assert_buffer(got, ref, f"attention_relpos {case}")
    assert np.array_equal(_launch(a, d, ref[0].shape).view(np.uint16), got.view(np.uint16)), "a second call gave other bits"


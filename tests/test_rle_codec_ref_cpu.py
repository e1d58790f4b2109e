"""tests/rle_codec_ref.py against vectors that can be checked by hand, and what the codec's entries refuse before anything touches a device. No GPU."""
import ctypes as C

import numpy as np
import pytest

from tests import rle_codec_ref as ref
from visioncpp_amd import _lib as L
from visioncpp_amd import vision

_buf = C.create_string_buffer(4096)
P = (C.addressof(_buf) + 15) & ~15  # 16-byte aligned zeros, never written: every call below is refused first

SINGLE = {0: "0", 15: "?", 16: "`0", 31: "o0", 32: "P1", 511: "o?", 512: "P`0", 1048576: "PPPP1", 2147483647: "oooooo1"}
DELTA = {-1: "O", -16: "@", -17: "_O", -512: "P@", -513: "o_O", -2147483646: "RPPPPPN"}
RECORD = [([5, 3, 7, 3, 7, 2, 39], "53700OP1"), ([0, 6, 1, 2, 17, 600, 1, 0, 70000], "061L`0fb0@X]O_[T2")]
MALFORMED = {1: "53~0", 2: "537P", 3: "5PPPPPPP03", 4: "537@"}  # 126 is no byte of the code; ends in a group with bit 5; eight bytes; the fourth run is 3 - 16


def test_vectors():
    for v, s in SINGLE.items():
        assert ref.enc([v]) == s.encode() and ref.dec(s) == [v]
    for d, s in DELTA.items():
        row = [0, max(0, -d), 0, max(0, -d) + d]  # the fourth run is the first delta
        assert ref.enc(row) == ref.enc(row[:3]) + s.encode() and ref.dec(ref.enc(row)) == row
    for row, s in RECORD:
        assert ref.enc(row) == s.encode() and ref.dec(s) == row


def test_reference_round_trip_on_random_rows():
    rng = np.random.default_rng(5)
    for n in (0, 1, 2, 3, 4, 50, 400):
        row = (rng.integers(0, 2 ** 31, n) >> rng.integers(0, 31, n)).tolist()
        s = ref.enc(row)
        assert ref.dec(s) == row and all(48 <= b <= 111 for b in s) and n <= len(s) <= 7 * n


def test_entries_refuse_before_any_device_call():
    api = L.get_lib()
    off, runs = np.array([0, 2, 3], np.int64), np.array([5, 2 ** 31, 7], np.uint32)
    o, r = off.ctypes.data, runs.ctypes.data
    for args, msg in [((None, r, 2, P, P, P, None), "null"), ((o, None, 2, P, P, P, None), "null"), ((o, r, 2, None, P, P, None), "null"), ((o, r, 2, P, None, P, None), "null"),
                      ((o, r, 2, P, P, None, None), "null"), ((o, r, 0, P, P, P, None), "0 records"), ((o, r, 2, P, P, P, None), "run 1 of record 0 is 2147483648")]:
        with pytest.raises(L.Error, match=f"rle_compress.*{msg}"):
            L.check(api.visp_image_rle_compress_host(*args))
    for args, msg in [((None, P, 1, P, P, P, None), "null"), ((P, None, 1, P, P, P, None), "null"), ((P, P, 1, None, P, P, None), "null"), ((P, P, 1, P, P, None, None), "null"),
                      ((P, P, 0, P, P, P, None), "0 records")]:
        with pytest.raises(L.Error, match=f"rle_decompress.*{msg}"):
            L.check(api.visp_image_rle_decompress_host(*args))
    for fn, args in [("compress", (None, P, 1, None, P, P, P, None, None)), ("compress", (P, P, 1, None, None, None, None, None, None)), ("compress", (P, P, 70000, None, P, P, P, None, None)),
                     ("decompress", (None, P, 1, None, P, P, P, None, None, None)), ("decompress", (P, P, 1, None, P, None, P, None, None, None)),
                     ("decompress", (P, P, 0, None, P, P, P, None, None, None))]:
        with pytest.raises(L.Error, match=f"rle_{fn}"):
            L.check(getattr(api, f"visp_image_rle_{fn}_device")(*args))
    for args in ((None, 1, 8, 8, P, P, P, None), (P, 0, 8, 8, P, P, P, None), (P, 1, 8, 0, P, P, P, None), (P, 1, 8, 8, None, P, P, None), (P, 1, 8, 8, P, None, P, None)):
        with pytest.raises(L.Error, match="rle_encode"):
            L.check(api.visp_image_rle_encode_compressed_host(*args))
    with pytest.raises(L.Error, match="null argument"):  # refused before the handle is looked at
        L.check(api.visp_sam_generate_masks_coco_rle_host(None, P, P, 1, 0.5, 0.5, 1.0, 0.7, 4, 0, P, P, P, P, None, P))
    assert api.vx_rle_compress_workspace_bytes(5000, 3) == 256 and api.vx_rle_compress_workspace_bytes(2 ** 31, 3) == 0
    for call in (lambda: api.vx_rle_compress(P, P, 0, 0, 1, None, 0, None, None, None, P, 4096, None), lambda: api.vx_rle_compress(P, P, 0, 0, 1, None, 0, P, None, P, P, 4096, None),
                 lambda: api.vx_rle_compress(P, P, 0, 0, 1, None, 0, None, None, P, P, 16, None), lambda: api.vx_rle_decompress(P, P, 0, None, 0, None, None, P, None, None),
                 lambda: api.vx_rle_decompress(P, P, 1, None, 0, P, None, P, None, None)):
        assert call() == 0 and b"vx_rle_" in api.vx_last_error()


@pytest.mark.parametrize("status", [1, 2, 3, 4])
def test_rle_decompress_refuses_a_malformed_record(status):
    bad = MALFORMED[status]
    at = {1: 2, 2: 3, 3: 8, 4: 3}[status]  # the byte the loop stands on when it meets the fault
    with pytest.raises(L.Error, match=f"rle_decompress: record 1, byte {at}: status {status}"):
        vision.rle_decompress([{"size": [3, 5], "counts": b"537"}, {"size": [3, 5], "counts": bad}])

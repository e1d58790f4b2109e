"""vx_mask_remove_small_regions_u8 (csrc/kernels_regions.hip) on the device against tests/sam_regions_ref.py. Every mask byte and every `changed` flag must
be EQUAL to the reference: there is nothing to tolerate. The mask buffer carries canaries before and behind and is compared whole; `changed` and the
workspace carry canaries behind; every call runs twice on fresh buffers and must give the same bytes. T is the kernel's tile edge (32)."""
import numpy as np
import pytest

from tests import gpu_util as G
from tests import sam_regions_cases as SC
from tests import sam_regions_ref as RR

pytestmark = pytest.mark.gpu

CANARY_I, CANARY_B = -7777, 7
GUARD = 64
T = SC.T

REPORT = G.Report("region kernels: {launches} calls in {seconds:.1f} s; masks and flags compared for equality:", lambda key, ratio, count: f"  {key:<40} {count} calls")
_device = G.device_fixture(REPORT)
_release_buffers = G.release_fixture()


def _api():
    from visioncpp_amd import _lib as L
    return L, G.api()


def run(masks, min_area, mode, counts=None, group=None, with_changed=True):
    """the launcher on masks [n, h, w] -> (masks, changed [n]) with the untouched ranges asserted; twice, equal bytes"""
    L, api = _api()
    n, h, w = masks.shape
    group = group or n
    ws_bytes = api.vx_mask_regions_workspace_bytes(w, h, group)
    assert ws_bytes >= 8 * group * w * h
    cd = G.dev(np.array([counts, 12345], np.int32)) if counts is not None else None
    runs = []
    for _ in range(2):
        buf = np.concatenate([np.full(GUARD, CANARY_B, np.uint8), masks.reshape(-1), np.full(GUARD, CANARY_B, np.uint8)])
        md, ch, ws = G.dev(buf), G.dev(np.full(n + GUARD, CANARY_I, np.int32)), G.dev(np.full(ws_bytes + GUARD, CANARY_B, np.uint8))
        L.vx_check(api.vx_mask_remove_small_regions_u8(md.ptr + GUARD, w, h, n, cd.ptr if cd else None, min_area, mode, ch.ptr if with_changed else None, ws.ptr, ws_bytes,
                                                       group, None))
        G.sync()
        assert (ws.to_numpy(np.uint8, (ws_bytes + GUARD,))[ws_bytes:] == CANARY_B).all(), "written behind the workspace"
        runs.append((md.to_numpy(np.uint8, (buf.size,)), ch.to_numpy(np.int32, (n + GUARD,))))
    assert runs[0][0].tobytes() == runs[1][0].tobytes() and runs[0][1].tobytes() == runs[1][1].tobytes(), "the same call twice gave other bytes"
    got, changed = runs[0]
    assert (got[:GUARD] == CANARY_B).all() and (got[-GUARD:] == CANARY_B).all(), "written before or behind the masks"
    assert (changed[n:] == CANARY_I).all(), "written behind the flags"
    return got[GUARD:-GUARD].reshape(n, h, w), changed[:n]


def check(masks, min_area, mode, what, **kw):
    want, want_changed = RR.remove_small_regions(masks, min_area, mode)
    got, changed = run(masks, min_area, mode, **kw)
    bad = np.argwhere(got != want)
    assert not len(bad), f"{what}: {len(bad)} bytes differ, the first at (mask, y, x) = {bad[0].tolist()}: got {got[tuple(bad[0])]}, want {want[tuple(bad[0])]}"
    assert changed.tolist() == want_changed.tolist(), f"{what}: changed {changed.tolist()}, want {want_changed.tolist()}"
    REPORT.add(what.split(" mode")[0], 0.0, 2)
    return want, want_changed


CASES = SC.named_cases()


@pytest.mark.parametrize("mode", [RR.HOLES, RR.ISLANDS, RR.BOTH], ids=["holes", "islands", "both"])
@pytest.mark.parametrize("name", list(CASES))
def test_remove_small_regions(name, mode):
    masks, min_area = CASES[name]
    check(masks, min_area, mode, f"{name} mode {mode}")


def test_the_named_cases_do_what_their_names_say():
    """on the device's own output (the CPU test asserts the same of the reference)"""
    got, ch = run(SC.two_equal_small_islands()[None], 9, RR.ISLANDS)
    assert ch.tolist() == [1] and (got[0, 2:4, 3:5] == 255).all() and int((got != 0).sum()) == 4
    m = SC.hole_between_islands()[None]
    both, ch = run(m, 20, RR.BOTH)
    assert ch.tolist() == [1] and (both[0, 0:5] == 255).all() and (both[0, 5:26] == 0).all() and (both[0, 26:] == 255).all()
    isl, _ = run(m, 20, RR.ISLANDS)
    assert (isl[0, 0:26] == 0).all() and (isl[0, 26:] == 255).all()
    got, ch = run(SC.hole_at_border()[None], 5, RR.HOLES)
    assert ch.tolist() == [1] and (got == 255).all()
    got, ch = run(SC.exact_area(7)[None], 7, RR.BOTH)
    assert (got[0, 1, 1:8] == 255).all() and (got[0, 3] == 0).all() and (got[0, 7, 2:9] == 0).all() and (got[0, 9] == 255).all()
    for m in (SC.checkerboard(2 * T + 3, T + 5), SC.diagonal(3 * T + 2, 3 * T + 2)):
        got, ch = run(m[None], int((m != 0).sum()), RR.ISLANDS)  # one component of exactly min_area pixels: it stays
        assert ch.tolist() == [0] and (got[0] == m).all()


def test_a_serpentine_through_every_tile_of_1024_squared():
    """one component of 524799 pixels that passes all 1024 tiles, and 511 background rows of 1023 pixels: no iteration count bounds the merge"""
    s = SC.serpentine(1024, 1024)[None]
    want, ch = check(s, 524799, RR.ISLANDS, "serpentine 1024 stays mode 2")
    assert ch.tolist() == [0]
    want, ch = check(s, 524800, RR.BOTH, "serpentine 1024 filled mode 3")
    assert ch.tolist() == [1] and (want == 255).all()
    want, ch = check(s, 1024, RR.HOLES, "serpentine 1024 rows filled mode 1")
    assert ch.tolist() == [1] and (want[0, :1023] == 255).all()


@pytest.mark.parametrize("min_area", [0, 1])
def test_min_area_0_and_1_write_no_byte(min_area):
    masks = np.stack([SC.random_mask(T + 9, T + 2, 0.5, seed=9, values=(1, 77, 255)), SC.checkerboard(T + 9, T + 2)])
    got, changed = run(masks, min_area, RR.BOTH)
    assert got.tobytes() == masks.tobytes() and changed.tolist() == [0, 0]


@pytest.mark.parametrize("group", [1, 2, 5])
def test_masks_behind_the_count_are_untouched_in_groups(group):
    """n = 5 with counts[0] = 3: masks 3 and 4 and their flags stay; the groups of 1 and 2 pass the workspace three and two times"""
    masks = np.stack([SC.random_mask(2 * T + 3, T + 5, d, seed=i) for i, d in enumerate((0.2, 0.5, 0.8, 0.5, 0.3))])
    want, want_changed = RR.remove_small_regions(masks[:3], 9, RR.BOTH)
    got, changed = run(masks, 9, RR.BOTH, counts=3, group=group)
    assert got[:3].tobytes() == want.tobytes() and got[3:].tobytes() == masks[3:].tobytes()
    assert changed[:3].tolist() == want_changed.tolist() == [1, 1, 1] and changed[3:].tolist() == [CANARY_I, CANARY_I]
    full, full_changed = run(masks, 9, RR.BOTH, group=group)
    assert full.tobytes() == RR.remove_small_regions(masks, 9, RR.BOTH)[0].tobytes() and full_changed.tolist() == [1] * 5
    none, none_changed = run(masks, 9, RR.BOTH, counts=0, group=group)
    assert none.tobytes() == masks.tobytes() and (none_changed == CANARY_I).all()
    REPORT.add("counts and groups", 0.0, 6)


def test_the_flags_are_optional():
    masks = SC.random_mask(T + 1, T + 1, 0.4, seed=5)[None]
    got, changed = run(masks, 6, RR.BOTH, with_changed=False)
    assert got.tobytes() == RR.remove_small_regions(masks, 6, RR.BOTH)[0].tobytes() and changed.tolist() == [CANARY_I]


def test_the_launcher_refuses_bad_operands():
    L, api = _api()
    scratch = G.empty(1 << 16)
    p = scratch.ptr
    assert api.vx_mask_regions_workspace_bytes(8, 8, 2) == 2 * 512 + 256
    assert api.vx_mask_regions_workspace_bytes(0, 8, 1) == 0 and api.vx_mask_regions_workspace_bytes(8, 8, 0) == 0 and api.vx_mask_regions_workspace_bytes(65536, 65536, 1) == 0
    for args in (
        (None, 8, 8, 2, None, 4, 3, p, p, 1 << 16, 2, None),       # no masks
        (p, 8, 8, 2, None, 4, 3, p, None, 1 << 16, 2, None),       # no workspace
        (p, 0, 8, 2, None, 4, 3, p, p, 1 << 16, 2, None),          # empty extent
        (p, 8, 0, 2, None, 4, 3, p, p, 1 << 16, 2, None),
        (p, 8, 8, 0, None, 4, 3, p, p, 1 << 16, 2, None),          # no mask
        (p, 8, 8, 2, None, 4, 3, p, p, 1 << 16, 0, None),          # group 0
        (p, 8, 8, 2, None, -1, 3, p, p, 1 << 16, 2, None),         # negative min_area
        (p, 8, 8, 2, None, 4, 0, p, p, 1 << 16, 2, None),          # unknown mode
        (p, 8, 8, 2, None, 4, 4, p, p, 1 << 16, 2, None),
        (p, 8, 8, 2, None, 4, 3, p, p, 1279, 2, None),             # workspace too small
        (p, 8, 8, 2, None, 4, 3, p, p + 4, 1 << 15, 2, None),      # workspace not 16-byte aligned
    ):
        with pytest.raises(L.Error, match="vx_mask_remove_small_regions_u8"):
            L.vx_check(api.vx_mask_remove_small_regions_u8(*args))
    G.assert_nothing_launched(scratch, 1 << 16)

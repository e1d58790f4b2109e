"""The kernels of the batched MobileSAM decode (csrc/kernels_samprompts.hip) on the device against tests/sam_prompts_ref.py:

  vx_sam_iou_head_f32    against float64. Allowance: 8 x the largest distance of numpy's own float32 evaluation (k ascending) from float64 over the same
                         cases -- the kernel's sums are float32 chains too, in another order (64 lanes, then a butterfly), and the factor covers the order.
                         `chosen` is exact wherever the float64 gap between the two best of the first three exceeds that allowance, and is the first index
                         where two predictions are the same bits.
  vx_sam_process_masks   byte-equal to two vx_sam_interpolate calls per prompt on the plane `chosen` names.
  vx_sam_tile_rows_f16   copies, bit for bit.
Every output buffer starts filled with a canary and is compared whole (tests/buffer_check.py): nothing behind the written ranges may change. The module's
teardown prints the figures profiles/sam_prompt_batch_ratios.txt records."""
import numpy as np
import pytest

from tests import buffer_check as BC
from tests import gpu_util as G
from tests import sam_prompts_ref as R

pytestmark = pytest.mark.gpu

CANARY = -24000.0
GUARD = 64
FIGURES = {}


def _report_tail():
    return [f"  {k}: {v}" for k, v in FIGURES.items()]


REPORT = G.Report("sam prompt kernels: {launches} launches in {seconds:.1f} s; largest |got - float64| / allowance per kernel and case:",
                  lambda key, ratio, count: f"  {key[0]:<24} {key[1]:<8} {ratio:.3f}", _report_tail)
_device = G.device_fixture(REPORT)
_release_buffers = G.release_fixture()

IOU_CASES = R.iou_head_cases()


@pytest.fixture(scope="module")
def iou_allowance():
    """8 x the largest |numpy float32 (k ascending) - float64| over the cases: the error a float32 evaluation of these sums makes, times the margin for
    another summation order. Derived from the reference side alone."""
    err = max(float(np.abs(R.iou_head_f32_ascending(t, ws, bs).astype(np.float64) - R.iou_head(t, ws, bs)).max()) for _, t, ws, bs in IOU_CASES)
    assert err > 0
    FIGURES["numpy float32 (k ascending) against float64, largest over the cases"] = f"{err:.3e}"
    FIGURES["allowance of vx_sam_iou_head_f32 (8 x that)"] = f"{8 * err:.3e}"
    return 8 * err


def _launch_iou(tokens, stride, ws, bs, iou, chosen):
    P = tokens.shape[0]
    rows = np.zeros((P, stride), np.float16)
    rows[:, : tokens.shape[1]] = tokens
    rows[:, tokens.shape[1]:] = np.float16(777.0)  # the gap between token rows is not part of the token
    t = G.dev(rows)
    d = [G.dev(a) for pair in zip(ws, bs) for a in pair]
    from visioncpp_amd import _lib as L
    L.vx_check(G.api().vx_sam_iou_head_f32(t.ptr, stride, P, *[b.ptr for b in d], ws[0].shape[1], ws[0].shape[0], ws[1].shape[0], ws[2].shape[0], iou.ptr,
                                           chosen.ptr if chosen is not None else None, None))
    G.sync()


@pytest.mark.parametrize("case", IOU_CASES, ids=lambda c: c[0])
def test_iou_head(case, iou_allowance):
    name, tokens, ws, bs = case
    P, N2 = tokens.shape[0], ws[2].shape[0]
    want64 = R.iou_head(tokens, ws, bs)
    size = P * N2 + GUARD
    want, allow, written = np.full(size, CANARY), np.zeros(size), np.zeros(size, bool)
    want[: P * N2], allow[: P * N2], written[: P * N2] = want64.reshape(-1), iou_allowance, True
    runs = []
    for _ in range(2):
        iou, chosen = G.dev(np.full(size, CANARY, np.float32)), G.dev(np.full(P + GUARD, -7, np.int32))
        _launch_iou(tokens, 7 * 256, ws, bs, iou, chosen)
        runs.append((iou.to_numpy(np.float32, (size,)), chosen.to_numpy(np.int32, (P + GUARD,))))
    got, got_chosen = runs[0]
    v = BC.assert_buffer(got, (want, allow, written), f"vx_sam_iou_head_f32 {name}", untouched=CANARY)
    REPORT.add(("vx_sam_iou_head_f32", name), v["ratio"], 2)
    FIGURES[f"vx_sam_iou_head_f32 {name}: largest |got - float64|"] = f"{v['err']:.3e}"
    assert (got_chosen[P:] == -7).all(), "chosen: written behind the last prompt"
    assert got.tobytes() == runs[1][0].tobytes() and got_chosen.tobytes() == runs[1][1].tobytes(), "the same call twice gave other bytes"
    top = np.sort(want64[:, :3], axis=1)
    decided = (top[:, 2] - top[:, 1]) > iou_allowance
    assert decided.any() or name == "tie"
    np.testing.assert_array_equal(got_chosen[:P][decided], R.choose(want64)[decided])
    np.testing.assert_array_equal(got_chosen[:P], R.choose(got[: P * N2].reshape(P, N2)))  # the rule itself, on the device's own numbers
    if name == "tie":
        g = got[: P * N2].reshape(P, N2)
        assert g[:, 0].tobytes() == g[:, 1].tobytes() and (got_chosen[:P] == 0).all()
    if name == "close":
        g = got[: P * N2].reshape(P, N2)
        assert (g[:, 1] > g[:, 0]).all() and np.abs((g[:, 1] - g[:, 0]) - 1e-4).max() < 3e-5 and (got_chosen[:P] == 1).all()


def test_iou_head_without_chosen_and_refusals(iou_allowance):
    from visioncpp_amd import _lib as L
    _, tokens, ws, bs = IOU_CASES[0]
    iou = G.dev(np.full(4 + GUARD, CANARY, np.float32))
    _launch_iou(tokens, 256, ws, bs, iou, None)
    got = iou.to_numpy(np.float32, (4 + GUARD,))
    assert np.abs(got[:4] - R.iou_head(tokens, ws, bs)[0]).max() <= iou_allowance and (got[4:] == CANARY).all()
    scratch = G.empty(4096)
    p = scratch.ptr
    for args in ((p, 255, 1, p, p, p, p, p, p, 256, 256, 256, 4, p, p, None),      # row stride below the width
                 (p, 256, 0, p, p, p, p, p, p, 256, 256, 256, 4, p, p, None),      # no prompt
                 (p, 256, 1, p, p, p, p, p, p, 256, 256, 256, 2, p, p, None),      # fewer than three predictions
                 (p, 2048, 1, p, p, p, p, p, p, 2048, 256, 256, 4, p, p, None),    # wider than the kernel's LDS rows
                 (p, 256, 1, p, p, None, p, p, p, 256, 256, 256, 4, p, p, None)):  # a null weight
        with pytest.raises(L.Error, match="vx_sam_iou_head_f32"):
            L.vx_check(G.api().vx_sam_iou_head_f32(*args))
    G.assert_nothing_launched(scratch, 4096)


@pytest.fixture(scope="module")
def planes():
    rng = np.random.default_rng(41)
    yy, xx = np.meshgrid(np.linspace(-3, 3, 256), np.linspace(-3, 3, 256), indexing="ij")
    base = np.sin(2 * xx) * np.cos(3 * yy)
    p = np.stack([np.stack([(1 + 0.2 * c) * np.roll(base, 17 * c + 5 * q, axis=q % 2) + 0.3 * rng.standard_normal((256, 256)) for c in range(8)], axis=-1)
                  for q in range(3)])
    return p.reshape(3, 256 * 256, 8).astype(np.float16)  # [P][256^2][8]: the layout of the single-prompt mask product, plane = column


@pytest.mark.parametrize("tw,th", [(1024, 1024), (640, 480), (333, 517)])
def test_process_masks_equals_two_interpolate_calls_per_prompt(planes, tw, th):
    from visioncpp_amd import _lib as L
    P, S, M = 3, 1024, 256
    chosen = np.random.default_rng(tw).integers(0, 4, P).astype(np.int32)
    if tw == 640:
        chosen[:] = [3, 0, 2]
    src, ch = G.dev(planes), G.dev(chosen)
    up = np.float32(S) / np.float32(max(tw, th))
    sw, sh = int(np.float32(tw) * up + np.float32(0.5)), int(np.float32(th) * up + np.float32(0.5))
    runs = []
    for _ in range(2):
        scaled, out = G.empty(P * S * S * 4), G.dev(np.full(P * tw * th + GUARD, 7, np.uint8))
        L.vx_check(G.api().vx_sam_process_masks(src.ptr, M * M * 8, 1, 8, M, 4, ch.ptr, scaled.ptr, S, sw, sh, out.ptr, tw, th, P, None))
        G.sync()
        runs.append(out.to_numpy(np.uint8, (P * tw * th + GUARD,)))
    got = runs[0]
    assert (got[P * tw * th:] == 7).all(), "written behind the last mask"
    assert got.tobytes() == runs[1].tobytes()
    got = got[: P * tw * th].reshape(P, th, tw)
    assert set(np.unique(got)) <= {0, 255}
    one_scaled, one_out = G.empty(S * S * 4), G.empty(tw * th)
    for p in range(P):
        L.vx_check(G.api().vx_sam_interpolate(src.ptr + (p * M * M * 8 + int(chosen[p])) * 2, 1, M, M, M, 8, one_scaled.ptr, S, S, 0, None))
        L.vx_check(G.api().vx_sam_interpolate(one_scaled.ptr, 0, sw, sh, S, 1, one_out.ptr, tw, th, 1, None))
        G.sync()
        np.testing.assert_array_equal(got[p], one_out.to_numpy(np.uint8, (th, tw)), err_msg=f"prompt {p}, plane {chosen[p]}")
    ref = R.process_masks(planes.reshape(P, M, M, 8).transpose(0, 3, 1, 2).astype(np.float32), chosen, tw, th)
    differing = float((got != ref).mean())
    REPORT.add(("vx_sam_process_masks", f"{tw}x{th}"), 0.0, 2)
    FIGURES[f"vx_sam_process_masks {tw}x{th}: pixels differing from the numpy restatement"] = f"{differing:.2e}"
    assert differing < 1e-5, differing


def test_process_masks_clamps_chosen_and_refuses_bad_operands(planes):
    from visioncpp_amd import _lib as L
    P, S, M, tw, th = 3, 1024, 256, 64, 48
    src = G.dev(planes)
    outs = []
    for chosen in ([9, -3, 1], [3, 0, 1]):
        scaled, out = G.empty(P * S * S * 4), G.empty(P * tw * th)
        L.vx_check(G.api().vx_sam_process_masks(src.ptr, M * M * 8, 1, 8, M, 4, G.dev(np.array(chosen, np.int32)).ptr, scaled.ptr, S, S, 768, out.ptr, tw, th, P, None))
        G.sync()
        outs.append(out.to_numpy(np.uint8, (P, th, tw)))
    np.testing.assert_array_equal(outs[0], outs[1])
    scratch = G.empty(4096)
    p = scratch.ptr
    for args in ((p, 8, 1, 8, 4, 4, p, p, 8, 8, 8, p, 4, 4, 0, None),      # no prompt
                 (p, 8, 1, 8, 4, 4, None, p, 8, 8, 8, p, 4, 4, 1, None),   # no chosen
                 (p, 8, 1, 8, 4, 4, p, p, 8, 9, 8, p, 4, 4, 1, None),      # crop wider than the map
                 (p, 8, 1, 0, 4, 4, p, p, 8, 8, 8, p, 4, 4, 1, None)):     # step 0
        with pytest.raises(L.Error, match="vx_sam_process_masks"):
            L.vx_check(G.api().vx_sam_process_masks(*args))
    G.assert_nothing_launched(scratch, 4096)


@pytest.mark.parametrize("n,B", [(8, 1), (4096 + 8, 3), (256 * 300 + 24, 2)])
def test_tile_rows(n, B):
    from visioncpp_amd import _lib as L
    src = np.random.default_rng(n).standard_normal(n).astype(np.float16)
    dst = G.dev(np.full(B * n + GUARD, CANARY, np.float16))
    L.vx_check(G.api().vx_sam_tile_rows_f16(G.dev(src).ptr, n, dst.ptr, B, None))
    G.sync()
    got = dst.to_numpy(np.float16, (B * n + GUARD,))
    assert got[: B * n].tobytes() == np.tile(src, B).tobytes()
    assert (got[B * n:] == np.float16(CANARY)).all()
    REPORT.add(("vx_sam_tile_rows_f16", f"n{n}"), 0.0)
    with pytest.raises(L.Error, match="vx_sam_tile_rows_f16"):
        L.vx_check(G.api().vx_sam_tile_rows_f16(dst.ptr, 12, dst.ptr, 1, None))

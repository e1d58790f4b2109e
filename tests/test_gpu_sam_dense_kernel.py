"""csrc/kernels_samdense.hip on the device against tests/sam_dense_ref.py.

  vx_sam_dense_prompt_f16   K against float64 with the kernel's two declared roundings. Allowance: one f16 ulp at the result, plus 8 x the largest distance of
                            numpy's own float32 evaluation from float64 over the same cases (before the last rounding): the kernel's stages are float32 chains
                            too, in another order, and a stage-2 activation that rounds to the other f16 neighbour is part of that distance on both sides.
                            Derived from the reference side alone. k1 must be f16(K as the kernel stored it + pe), bit for bit.
  vx_sam_gather_plane_f32, vx_sam_fix_plane_i32   exact.
Every output buffer starts filled with a canary and is compared whole (tests/buffer_check.py). The teardown prints what profiles/sam_dense_prompt_ratios.txt records."""
import numpy as np
import pytest

from tests import buffer_check as BC
from tests import gpu_util as G
from tests import sam_dense_ref as R

pytestmark = pytest.mark.gpu

CANARY = -24000.0
GUARD = 64
# (n, res, dim, pe given, mask row stride - 4 res, embedding f32): one MFMA tile; 75 rows = a tail of 11 and three channel tiles; the real shape; a padded
# mask row stride with 17 channel tiles (a second channel group of one tile) and a tail
CASES = [(1, 4, 16, False, 0, False), (3, 5, 48, True, 0, False), (2, 64, 256, True, 0, True), (2, 5, 272, True, 8, True)]
IDS = ["one_tile", "tail_3tiles", "real", "padded_stride_17tiles"]

REPORT = G.Report("sam dense prompt kernel: {launches} launches in {seconds:.1f} s; largest |got - float64| / allowance per case:",
                  lambda key, ratio, count: f"  {key:<24} {ratio:.3f}")
_device = G.device_fixture(REPORT)
_release_buffers = G.release_fixture()


def _operands(case):
    from visioncpp_amd import synth
    n, res, dim, with_pe, pad, embed_f32 = case
    rng = np.random.default_rng(1000 * res + dim)
    W = R.weights(synth.sam_decoder_state_dict(7, dim=dim, mlp_dim=32, depth=0, mask_input=True))
    mask = (6 * rng.standard_normal((n, 4 * res, 4 * res))).astype(np.float32)
    embed = rng.standard_normal((res * res, dim)).astype(np.float32 if embed_f32 else np.float16)
    pe = rng.standard_normal((res * res, dim)).astype(np.float16) if with_pe else None
    return W, mask, embed, pe


@pytest.fixture(scope="module")
def references():
    """per case the operands and the float64 result; and the allowance's second term, from the float32 evaluation of all cases"""
    refs, err = [], 0.0
    for case in CASES:
        W, mask, embed, pe = _operands(case)
        raw64, K64 = R.dense_prompt(mask, W, embed)
        raw32, _ = R.dense_prompt(mask, W, embed, np.float32)
        err = max(err, float(np.abs(raw32.astype(np.float64) - raw64).max()))
        refs.append((W, mask, embed, pe, K64))
    assert err > 0
    print(f"numpy float32 against float64 over the cases: {err:.3e}; allowance: one f16 ulp + {8 * err:.3e}")
    return refs, 8 * err


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_dense_prompt(i, references):
    from visioncpp_amd import _lib as L
    refs, slack = references
    n, res, dim, with_pe, pad, embed_f32 = CASES[i]
    W, mask, embed, pe, K64 = refs[i]
    S, rows = 4 * res, n * res * res
    padded = np.full((n, S, S + pad), 1e30, np.float32)  # what stands between the rows is not part of the mask
    padded[:, :, :S] = mask
    f32 = lambda a: G.dev(np.ascontiguousarray(a, np.float32)).ptr
    size = rows * dim + GUARD
    K, k1 = G.dev(np.full(size, CANARY, np.float16)), G.dev(np.full(size, CANARY, np.float16))
    L.vx_check(G.api().vx_sam_dense_prompt_f16(
        G.dev(padded).ptr, S * (S + pad), S + pad, f32(W["0.weight"]), f32(W["0.bias"]), f32(W["1.weight"]), f32(W["1.bias"]), 4, f32(W["3.weight"]), f32(W["3.bias"]),
        f32(W["4.weight"]), f32(W["4.bias"]), 16, G.dev(W["6.weight"].reshape(dim, 16).astype(np.float16)).ptr, f32(W["6.bias"]), G.dev(embed).ptr, int(embed_f32),
        G.dev(pe).ptr if with_pe else None, K.ptr, k1.ptr if with_pe else None, n, res, dim, R.EPS, None))
    G.sync()
    got, got1 = K.to_numpy(np.float16, (size,)), k1.to_numpy(np.float16, (size,))
    want, allow, written = np.full(size, CANARY), np.zeros(size), np.zeros(size, bool)
    want[: rows * dim] = K64.astype(np.float64).reshape(-1)
    allow[: rows * dim] = np.spacing(np.abs(K64).reshape(-1)).astype(np.float64) + slack
    written[: rows * dim] = True
    v = BC.assert_buffer(got, (want, allow, written), f"vx_sam_dense_prompt_f16 {IDS[i]}", untouched=CANARY)
    REPORT.add(IDS[i], v["ratio"])
    want1 = np.full(size, CANARY, np.float16)
    if with_pe:
        want1[: rows * dim] = R.k1_of(got[: rows * dim].reshape(n, res * res, dim), pe).reshape(-1)
    assert got1.tobytes() == want1.tobytes(), "k1 is not f16(K as stored + pe), or something behind it was written"


def test_dense_prompt_refusals():
    from visioncpp_amd import _lib as L
    scratch = G.empty(1 << 16)
    p = scratch.ptr
    ok = [p, 256, 16, p, p, p, p, 4, p, p, p, p, 16, p, p, p, 0, p, p, p, 1, 4, 16, 1e-6, None]
    for at, bad in ((7, 8), (12, 32), (22, 24), (2, 18), (17, None), (0, None), (0, p + 4)):  # stage widths, dim, row stride, pe without k1, no mask, misaligned mask
        args = list(ok)
        args[at] = bad
        with pytest.raises(L.Error, match="vx_sam_dense_prompt_f16"):
            L.vx_check(G.api().vx_sam_dense_prompt_f16(*args))
    G.assert_nothing_launched(scratch, 1 << 16)


def test_gather_plane_and_fix_plane_are_exact():
    from visioncpp_amd import _lib as L
    P, n_px = 5, 300
    planes = np.random.default_rng(3).standard_normal((P, 4, n_px)).astype(np.float16)
    chosen = np.array([0, 1, 2, 3, 2], np.int32)
    out = G.dev(np.full(P * n_px + GUARD, CANARY, np.float32))
    L.vx_check(G.api().vx_sam_gather_plane_f32(G.dev(planes).ptr, 4 * n_px, n_px, n_px, 4, G.dev(chosen).ptr, out.ptr, P, None))
    G.sync()
    want = np.full(P * n_px + GUARD, CANARY, np.float32)
    want[: P * n_px] = planes[np.arange(P), chosen].astype(np.float32).reshape(-1)
    assert out.to_numpy(np.float32, (P * n_px + GUARD,)).tobytes() == want.tobytes()
    REPORT.add("gather_plane", 0.0)
    fixed = G.dev(np.full(P + GUARD, -7, np.int32))
    L.vx_check(G.api().vx_sam_fix_plane_i32(fixed.ptr, 3, P, None))
    G.sync()
    assert fixed.to_numpy(np.int32, (P + GUARD,)).tolist() == [3] * P + [-7] * GUARD

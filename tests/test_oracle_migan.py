"""CPU: the MI-GAN oracle (tests/migan_ref.py, composed of the CPU oracle's primitives) pinned on golden vectors that the
reference's own torch Encoder / Synthesis produced (tests/golden/make_golden_migan.py), plus the pre / post processing on
hand-made cases."""
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
from __graft_entry__ import load_package  # noqa: E402

load_package()
import migan_ref  # noqa: E402
from visioncpp_amd import synth  # noqa: E402

GOLDEN = ROOT / "tests" / "golden"


def _golden_inputs(res: int, seed: int) -> np.ndarray:  # == make_golden_migan.inputs
    rng = np.random.default_rng(seed)
    rgb = synth.images(1, res, res, seed=seed)[0].astype(np.float32) / 255.0
    yy, xx = np.mgrid[0:res, 0:res]
    mask = ((np.abs(yy - res * rng.uniform(0.3, 0.7)) < res / 4) & (np.abs(xx - res * rng.uniform(0.3, 0.7)) < res / 5)).astype(np.float32)
    a = 1.0 - mask
    return np.concatenate([(a - 0.5)[..., None], a[..., None] * (rgb * 2 - 1)], -1)[None].astype(np.float32)


def _run(name: str):
    g = np.load(GOLDEN / f"{name}.npz")
    res = int(g["res"])
    sd = migan_ref.f16_rounded(synth.migan_state_dict(res, int(g["ch_base"]), int(g["ch_max"]), int(g["wseed"])))
    caps = {}
    out = migan_ref.generate(sd, _golden_inputs(res, int(g["iseed"])), res, caps)[0]
    return g, out, caps


def test_channel_table():
    assert synth.migan_channels(512) == [64, 128, 256, 512, 512, 512, 512, 512]
    assert synth.migan_channels(256) == [128, 256, 512, 512, 512, 512, 512]


def test_generator_r16_matches_reference_torch():
    g, out, caps = _run("migan_r16")
    np.testing.assert_allclose(out, g["out"], atol=1e-4, rtol=1e-4)
    np.testing.assert_allclose(caps["enc.out"][0], g["enc_out"], atol=1e-4, rtol=1e-4)
    for r in (16, 8, 4):
        np.testing.assert_allclose(caps[f"enc.feat{r}"][0], g[f"feat{r}"], atol=1e-4, rtol=1e-4)


def test_generator_r256_matches_reference_torch():
    g, out, caps = _run("migan_r256")
    np.testing.assert_allclose(out.reshape(-1)[g["out_idx"]], g["out"], atol=2e-4, rtol=1e-3)
    for r in (256, 64, 4):
        np.testing.assert_allclose(caps[f"enc.feat{r}"][0].reshape(-1)[g[f"feat{r}_idx"]], g[f"feat{r}"], atol=2e-4, rtol=1e-3)


def test_preprocess_formula_by_hand():
    """{a - 0.5, a (2 rgb/255 - 1)} with a = 1 - mask/255 (migan.cpp:142-159, invert_mask)."""
    img = np.zeros((4, 4, 3), np.uint8)
    img[..., 0], img[..., 1], img[..., 2] = 255, 0, 51
    mask = np.zeros((4, 4), np.uint8)
    mask[1, 2] = 255
    mask[3, 0] = 102
    x = migan_ref.preprocess(img, mask, 4)
    assert x.shape == (4, 4, 4)
    np.testing.assert_allclose(x[0, 0], [0.5, 1.0, -1.0, -0.6], atol=1e-6)  # a = 1
    np.testing.assert_allclose(x[1, 2], [-0.5, 0.0, 0.0, 0.0], atol=1e-6)  # a = 0: the hole
    a = 1 - 0.4
    np.testing.assert_allclose(x[3, 0], [a - 0.5, a, -a, -0.6 * a], atol=1e-6)
    rgba = np.concatenate([img, np.full((4, 4, 1), 7, np.uint8)], -1)
    np.testing.assert_array_equal(migan_ref.preprocess(rgba, mask, 4), x)  # a 4th channel is ignored


def test_postprocess_restores_the_original_mask():
    rgb = np.array([[[-1.0, 0.0, 1.0], [0.5, -0.5, 2.0]]] * 2, np.float32)  # 2 x 2
    mask = np.array([[0, 255], [17, 200]], np.uint8)
    out = migan_ref.postprocess(rgb, mask)
    assert out.shape == (2, 2, 4) and out.dtype == np.uint8
    np.testing.assert_array_equal(out[..., 3], mask)
    np.testing.assert_array_equal(out[0, 0, :3], [0, 127, 255])  # trunc(clamp(x/2 + 1/2) * 255)
    np.testing.assert_array_equal(out[0, 1, :3], [191, 63, 255])


def test_upsample_is_polyphase_2x2():
    """The zero-insertion x2 + 4x4 FIR (pad 2, crop) equals the 2x2-tap polyphase form the device kernel uses."""
    rng = np.random.default_rng(0)
    x = rng.standard_normal((1, 3, 5, 2)).astype(np.float32)
    f = rng.standard_normal((2, 1, 4, 4)).astype(np.float32)
    got = migan_ref.upsample(x, f)
    want = np.zeros((1, 6, 10, 2), np.float32)
    for Y in range(6):
        for X in range(10):
            for ky in range(Y & 1, 4, 2):
                for kx in range(X & 1, 4, 2):
                    iy, ix = (Y + ky - 2) // 2, (X + kx - 2) // 2
                    if 0 <= iy < 3 and 0 <= ix < 5:
                        want[0, Y, X] += x[0, iy, ix] * f[:, 0, ky, kx]
    np.testing.assert_allclose(got, want, atol=1e-5)

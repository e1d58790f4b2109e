"""-m gpu: the matting kernels (csrc/kernels_matting.hip) and the BiRefNet cutout against float64 on the same f32 inputs (tests/matting_ref.py). Every
output element is checked, and a guard region behind every output (and the padding of padded rows) must come back untouched.

Blur allowance, per element: K * 2^-24 * boxmean(|x|) + 2^-126 with K = 2 (2 r + 1) + 3, from the kernels' summation order. Each pass adds the
n = 2 r + 1 terms of the output's own window one after the other into an accumulator that starts at the first term (the vertical pass starts at 0.0f and
adds 0.0f for rows outside the window: exact), so sum' = sum_i x_i (1 + t_i) with |t_i| <= (n - 1) u, u = 2^-24; then one multiplication by fl(1 / n),
which carries the rounding of the weight and of the product: a pass is off by at most (n + 1) u * mean(|terms|). The second pass sums first-pass
outputs t_j with |t_j| <= mean_h(|x|) (1 + (n + 1) u): (n + 1) u of its own plus the (n + 1) u it carries over = 2 (n + 1) u * boxmean(|x|); the
second-order terms, (n + 1)^2 u^2 < 3e-4 u for n <= 65, are far inside the +1. K = 2 n + 3 <= 4 n for every legal radius (the issue's cap). 2^-126
covers a product that lands in the subnormal range.

Estimator allowance for the f32 output: (8 (n1 + n2) + 64) * 2^-24 with n1 = 2 radius + 1, n2 = 7 (3.6e-5 at radius 30): the summed terms are
non-negative, so bf and bb carry at most 2 (n + 1) u <= 4 n u relative error per stage, both are at most 1 (+1e-5 slack), the combine scales their
errors by at most (1 - m^2) + m (1 - m) <= 1.25, stage two is a weighted mean of stage one's values and carries their error over at most once; 64 u
covers the divisions, the combine's own roundings, the u8 / 255 loader and fl(1e-5). The kernels need no further term. u8 output: the reference's
truncating conversion of the float64 result, one level of slack only where 255 * result lies within 255 * allowance of a conversion boundary.

The tiles of the kernels: 256 threads per block over a linear index; strips of 4 rows per thread in the vertical passes (8 in the estimator's from radius
8 on) and of 4 columns in the estimator's horizontal launch from radius 8 on. Extents one below and one above a block and a strip of 4 are in the blur
cases; the estimator's extents leave remainders against 4 and 8 (131 x 67, 16 x 12, 37 x 21), and radii 7 and 8 run on both sides of the switch. Largest error / allowance per case is printed at module teardown (written to the file VISP_MATTING_RATIOS names);
profiles/matting_ratios.txt holds the MI355X's."""
import dataclasses
import os
import subprocess
from pathlib import Path

import numpy as np
import pytest

import matting_ref as R
from visioncpp_amd import _lib as L
from visioncpp_amd import synth, vision
from visioncpp_amd.vision import ImageFormat as F

pytestmark = pytest.mark.gpu

from gpu_util import api, dev, release, sync  # noqa: E402

ROOT = Path(__file__).resolve().parents[1]
U = 2.0 ** -24
GUARD = 1024        # bytes behind every output
GUARD_BYTE = 0x7B   # what guards and row padding are filled with
_ratios: list[str] = []


@pytest.fixture(scope="module")
def device():
    assert api().vx_device_count() > 0, "no HIP device visible: the product path has no CPU fallback"
    return vision.Device.init(vision.Backend.gpu)


@pytest.fixture(autouse=True)
def _release_buffers():
    yield
    release()


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    text = "\n".join(_ratios) + "\n"
    print("\n" + text)
    if os.environ.get("VISP_MATTING_RATIOS"):
        with open(os.environ["VISP_MATTING_RATIOS"], "w") as f:
            f.write(text)


@pytest.fixture(scope="module")
def vectors(golden_dir):
    import json

    return json.loads((golden_dir / "image_ops_vectors.json").read_text())


def guarded(nbytes):
    """A device buffer of nbytes + GUARD filled with GUARD_BYTE."""
    return dev(np.full(nbytes + GUARD, GUARD_BYTE, np.uint8))


def read_guarded(buf, dtype, shape):
    """The buffer's payload as dtype [shape]; asserts the guard behind it is untouched."""
    raw = buf.to_numpy(np.uint8, (buf.nbytes,))
    n = int(np.prod(shape)) * np.dtype(dtype).itemsize
    assert n + GUARD == buf.nbytes
    assert np.all(raw[n:] == GUARD_BYTE), "the guard region behind the output was written"
    return raw[:n].view(dtype).reshape(shape)


# ---- blur ----------------------------------------------------------------------------------------------------------------------------------------
def run_blur(x, radius, pad=0):
    """x f32 [B, h, w, C] -> (kernel output [B, h, w, C], in rows padded by `pad` pixels in and out)."""
    B, h, w, C = x.shape
    row = (w + pad) * C
    xin = np.full((B, h, w + pad, C), np.float32(7.5))
    xin[:, :, :w] = x
    out = guarded(B * h * row * 4)
    tmp = guarded(B * h * w * C * 4)
    L.vx_check(api().vx_box_blur_f32(dev(xin).ptr, row, tmp.ptr, out.ptr, row, B, h, w, C, radius, None))
    sync()
    read_guarded(tmp, np.float32, (B, h, w, C))
    got = read_guarded(out, np.float32, (B, h, w + pad, C))
    assert np.all(got[:, :, w:].view(np.uint8) == GUARD_BYTE), "row padding of the output was written"
    return got[:, :, :w]


def check_blur(name, x, radius, got):
    n = 2 * radius + 1
    K = 2 * n + 3
    assert K <= 4 * n
    worst = 0.0
    for b in range(x.shape[0]):
        want = R.box_blur(x[b], radius)
        allow = K * U * R.box_blur(np.abs(x[b]), radius) + 2.0 ** -126
        ratio = np.abs(got[b].astype(np.float64) - want) / allow
        worst = max(worst, float(ratio.max()))
    _ratios.append(f"vx_box_blur_f32 {name} r={radius}: largest error / allowance {worst:.3f} (K = {K})")
    assert worst <= 1.0, _ratios[-1]


BLUR_CASES = [(6, 6, 1), (7, 5, 2), (2, 2, 1), (64, 64, 30), (64, 64, 32), (130, 67, 3), (130, 67, 30), (257, 61, 30),
              (255, 3, 1), (257, 5, 2), (3, 257, 1), (85, 3, 1), (51, 5, 2)]  # 85 x 3 = 255, 51 x 5 = 255: one short of a block; RUN - 1 and RUN + 1 rows


@pytest.mark.parametrize("w,h,radius", BLUR_CASES)
@pytest.mark.parametrize("C", [1, 4])
@pytest.mark.parametrize("B,pad", [(1, 0), (3, 5)])
def test_box_blur_against_float64(w, h, radius, C, B, pad, vectors):
    rng = np.random.default_rng(w * 1000 + h * 10 + C + B)
    x = rng.uniform(-1, 1, (B, h, w, C)).astype(np.float32)
    if (w, h, radius) == (6, 6, 1):
        x[0, :, :, 0] = np.array(vectors["blur"]["input"], np.float32).reshape(6, 6)
    got = run_blur(x, radius, pad)
    if (w, h, radius) == (6, 6, 1):
        want = np.array(vectors["blur"]["expected"], np.float64).reshape(6, 6)
        assert np.sqrt(np.mean((got[0, :, :, 0] - want) ** 2)) <= 1e-5  # the reference's own test and criterion
    check_blur(f"{w}x{h} C={C} B={B} pad={pad}", x, radius, got)


def _adversarial(kind, n):
    v = np.full(n, 1e-4, np.float32)
    if kind == "bright_then_dim":
        v[:40] = 1.0
    elif kind == "dim_then_bright":
        v[-40:] = 1.0
    else:
        v[:] = 0.0
        v[n // 2 + 3] = 1.0
    return v


@pytest.mark.parametrize("kind", ["bright_then_dim", "dim_then_bright", "single_one"])
@pytest.mark.parametrize("along", ["rows", "columns"])
@pytest.mark.parametrize("C", [1, 4])
def test_box_blur_error_is_bounded_by_its_own_window(kind, along, C):
    """A running sum over the row carries the bright region's rounding into the dim outputs behind it and fails these; window-local sums pass."""
    n, m, radius = 200, 64, 30
    line = _adversarial(kind, n)
    plane = np.tile(line, (m, 1)) if along == "rows" else np.tile(line[:, None], (1, m))
    x = np.repeat(plane[None, :, :, None], C, axis=3).astype(np.float32)
    got = run_blur(x, radius)
    check_blur(f"{kind} along {along} C={C}", x, radius, got)
    if kind == "single_one":
        far = R.box_blur(x[0], radius) == 0
        assert np.all(got[0][far] == 0), "outputs whose window holds only zeros are exactly zero"


# ---- erosion -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h,radius", [(6, 6, 1), (7, 5, 2), (130, 67, 1), (130, 67, 5)])
@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
def test_erosion_is_bit_exact(w, h, radius, dtype, vectors):
    rng = np.random.default_rng(w + radius)
    B, pad = 2, 3
    x = rng.integers(0, 256, (B, h, w)).astype(np.uint8) if dtype == np.uint8 else rng.uniform(0, 1.5, (B, h, w)).astype(np.float32)
    if (w, h) == (6, 6):
        v = np.array(vectors["erosion"]["input"], np.float32).reshape(6, 6)
        x[0] = (v * 255).astype(np.uint8) if dtype == np.uint8 else v
    xin = np.zeros((B, h, w + pad), dtype)
    xin[:, :, :w] = x
    item = np.dtype(dtype).itemsize
    out = guarded(B * h * (w + pad) * item)
    fn = api().vx_erode_u8 if dtype == np.uint8 else api().vx_erode_f32
    L.vx_check(fn(dev(xin).ptr, w + pad, out.ptr, w + pad, B, h, w, radius, None))
    sync()
    got = read_guarded(out, dtype, (B, h, w + pad))
    assert np.all(got[:, :, w:].view(np.uint8) == GUARD_BYTE)
    for b in range(B):
        assert np.array_equal(got[b, :, :w], R.erosion(x[b], radius))
    if (w, h) == (6, 6) and dtype == np.float32:
        assert np.array_equal(got[0, :, :w], np.array(vectors["erosion"]["expected"], np.float32).reshape(6, 6))


# ---- composite -----------------------------------------------------------------------------------------------------------------------------------
def run_composite(fg, bg, mask):
    h, w = mask.shape
    out = guarded(h * w * 4)
    L.vx_check(api().vx_alpha_composite_u8(dev(fg).ptr, dev(bg).ptr, bg.shape[-1], dev(mask).ptr, out.ptr, h * w, None))
    sync()
    return read_guarded(out, np.uint8, (h, w, 4))


def test_alpha_composite_vector(vectors):
    v = vectors["alpha_composite"]
    fg = np.array(v["fg_rgba_u8"], np.uint8).reshape(2, 2, 4)
    bg = np.array(v["bg_rgb_u8"], np.uint8).reshape(2, 2, 3)
    mask = np.array(v["mask_u8"], np.uint8).reshape(2, 2)
    assert np.array_equal(run_composite(fg, bg, mask), np.array(v["expected_rgba_u8"], np.uint8).reshape(2, 2, 4))


@pytest.mark.parametrize("bg_channels", [3, 4])
def test_alpha_composite_is_exact(bg_channels):
    rng = np.random.default_rng(bg_channels)
    w, h = 131, 67
    fg = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    bg = rng.integers(0, 256, (h, w, bg_channels), dtype=np.uint8)
    mask = rng.integers(0, 256, (h, w), dtype=np.uint8)
    mask.reshape(-1)[:256] = np.arange(256, dtype=np.uint8)  # every weight occurs
    got = run_composite(fg, bg, mask)
    assert np.array_equal(got, R.alpha_composite(fg, bg, mask))
    assert np.array_equal(vision.image_alpha_composite(fg, bg, mask), got)  # the host-view entry on the current device


# ---- estimator -----------------------------------------------------------------------------------------------------------------------------------
def fg_allowance(radius):
    total = (8 * ((2 * radius + 1) + 7) + 64) * U
    assert total <= 2.0 ** -13
    return total


def make_mask(kind, w, h, rng):
    if kind == "step":
        m = np.zeros((h, w), np.float32)
        m[:, w // 2:] = 1.0
    elif kind == "ramp":
        m = np.tile(np.linspace(0, 1, w, dtype=np.float32), (h, 1))
    elif kind == "zeros":
        m = np.zeros((h, w), np.float32)
    elif kind == "ones":
        m = np.ones((h, w), np.float32)
    else:
        m = rng.random((h, w), dtype=np.float32)
    return m


def run_estimator(img, fmt, mask, radius, out_fmt):
    """img [B, h, w, c] (u8 or f32 by fmt), mask f32 [B, h, w] -> the output [B, h, w, 4] through the device-resident C entry."""
    B, h, w = mask.shape
    dtype = np.float32 if out_fmt is F.rgba_f32 else np.uint8
    out = guarded(B * h * w * 4 * np.dtype(dtype).itemsize)
    vision.estimate_foreground_batch_device(dev(img).ptr, fmt, dev(mask).ptr, B, w, h, out.ptr, out_fmt, radius)
    return read_guarded(out, dtype, (B, h, w, 4))


def check_foreground(name, got, out_fmt, want, radius):
    """want: float64 [.., 4]. f32 output within the allowance; u8 output = the truncating conversion, one level only next to a boundary."""
    allow = fg_allowance(radius)
    if out_fmt is F.rgba_f32:
        worst = float(np.abs(got.astype(np.float64) - want).max() / allow)
        _ratios.append(f"estimator {name} -> rgba_f32: largest error / allowance {worst:.3f}")
        assert worst <= 1.0, _ratios[-1]
    else:
        lo = np.floor(np.clip(want - allow, 0, 1) * 255.0)
        hi = np.floor(np.clip(want + allow, 0, 1) * 255.0)
        g = got.astype(np.float64)
        assert np.all((g >= lo) & (g <= hi)), f"estimator {name} -> rgba_u8: {int(((g < lo) | (g > hi)).sum())} values outside the conversion of the float64 result"


@pytest.mark.parametrize("kind", ["step", "ramp", "zeros", "ones", "random"])
@pytest.mark.parametrize("w,h,radius", [(64, 64, 30), (96, 80, 30), (131, 67, 30), (16, 12, 5)])
def test_estimator_against_float64(w, h, radius, kind):
    rng = np.random.default_rng(w + h + len(kind))
    mask = make_mask(kind, w, h, rng)
    img_f = rng.random((h, w, 4), dtype=np.float32)
    img_u = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    u_as_f32 = img_u[..., :3].astype(np.float32) / np.float32(255)  # what the loader makes of the bytes: the same f32 inputs
    want_f = R.estimate_foreground(img_f[..., :3], mask, radius)
    want_u = R.estimate_foreground(u_as_f32, mask, radius)
    inputs = [(F.rgba_f32, img_f, want_f), (F.rgb_u8, np.ascontiguousarray(img_u[..., :3]), want_u), (F.rgba_u8, img_u, want_u)]
    for fmt, img, want in inputs:
        for out_fmt in (F.rgba_f32, F.rgba_u8):
            got = run_estimator(img[None], fmt, mask[None], radius, out_fmt)[0]
            check_foreground(f"{w}x{h} r={radius} {kind} {fmt.name}", got, out_fmt, want, radius)
            if out_fmt is F.rgba_f32:
                assert np.array_equal(got[..., 3], np.clip(mask, 0, 1)), "alpha is the mask"
    # the host-view entry (rgba_f32 in, rgba_f32 out) on a strided view gives the device entry's bits
    wide = np.zeros((h, w + 3, 4), np.float32)
    wide[:, :w] = img_f
    host = vision.image_estimate_foreground(wide[:, :w], mask, radius)
    assert np.array_equal(host, run_estimator(img_f[None], F.rgba_f32, mask[None], radius, F.rgba_f32)[0])


def test_estimator_bits_repeat_and_do_not_depend_on_the_batch():
    rng = np.random.default_rng(5)
    B, w, h, radius = 3, 96, 80, 30
    img = rng.integers(0, 256, (B, h, w, 3), dtype=np.uint8)
    mask = rng.random((B, h, w), dtype=np.float32)
    for out_fmt in (F.rgba_f32, F.rgba_u8):
        a = run_estimator(img, F.rgb_u8, mask, radius, out_fmt)
        b = run_estimator(img, F.rgb_u8, mask, radius, out_fmt)
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), "two runs give equal bits"
        for i in range(B):
            alone = run_estimator(img[i:i + 1], F.rgb_u8, mask[i:i + 1], radius, out_fmt)[0]
            assert np.array_equal(alone.view(np.uint8), a[i].view(np.uint8)), f"image {i} of the batch differs from the image alone"


@pytest.mark.parametrize("radius", [4, 7, 8])  # 8 is where the launches start to work in strips
def test_foreground_stage_writes_the_blurred_background(radius):
    """vx_foreground_stage on its own, stage one: foreground and blurred background against float64, guards behind all three outputs."""
    rng = np.random.default_rng(9)
    B, w, h = 2, 37, 21
    img = rng.random((B, h, w, 4), dtype=np.float32)
    mask = rng.random((B, h, w), dtype=np.float32)
    planes, out, bg = guarded(B * h * w * 32), guarded(B * h * w * 16), guarded(B * h * w * 16)
    L.vx_check(api().vx_foreground_stage(dev(img).ptr, F.rgba_f32.value, None, None, dev(mask).ptr, planes.ptr, out.ptr, F.rgba_f32.value, bg.ptr, B, h, w, radius, 3, None))
    sync()
    both = read_guarded(planes, np.float32, (B, h, w, 8)).copy()
    f, bb = read_guarded(out, np.float32, (B, h, w, 4)), read_guarded(bg, np.float32, (B, h, w, 4))
    allow = (8 * (2 * radius + 1) + 64) * U  # one stage
    for b in range(B):
        rgb = img[b, ..., :3].astype(np.float64)
        want_f, want_b = R._stage(rgb, rgb, rgb, mask[b].astype(np.float64), radius)
        assert np.abs(f[b, ..., :3] - want_f).max() <= allow and np.abs(bb[b, ..., :3] - want_b).max() <= allow * 1.0001
        assert np.array_equal(f[b, ..., 3], mask[b]) and np.all(bb[b, ..., 3] == 0)
    # the two launches one at a time (what tools/bench_matting.py times) give the bits of the pair
    planes2, out2, bg2 = guarded(B * h * w * 32), guarded(B * h * w * 16), guarded(B * h * w * 16)
    for passes in (1, 2):
        L.vx_check(api().vx_foreground_stage(dev(img).ptr, F.rgba_f32.value, None, None, dev(mask).ptr, planes2.ptr, out2.ptr, F.rgba_f32.value, bg2.ptr, B, h, w, radius,
                                             passes, None))
        sync()
    assert np.array_equal(read_guarded(planes2, np.float32, (B, h, w, 8)), both)
    assert np.array_equal(read_guarded(out2, np.float32, (B, h, w, 4)), f) and np.array_equal(read_guarded(bg2, np.float32, (B, h, w, 4)), bb)


def test_host_view_blur_and_erosion_match_the_launchers(vectors):
    rng = np.random.default_rng(2)
    x = rng.uniform(-1, 1, (20, 31 + 4, 4)).astype(np.float32)
    view = x[:, 2:33]  # strided rows
    assert np.array_equal(vision.image_blur(view, 3), run_blur(np.ascontiguousarray(view)[None], 3)[0])
    a = rng.uniform(0, 1, (20, 31)).astype(np.float32)
    assert np.array_equal(vision.image_blur(a, 5), run_blur(a[None, :, :, None], 5)[0, :, :, 0])
    m8 = rng.integers(0, 256, (20, 40), dtype=np.uint8)[:, 4:35]
    assert np.array_equal(vision.image_erosion(m8, 2), R.erosion(m8, 2))
    assert np.array_equal(vision.image_erosion(a, 1), R.erosion(a, 1))


# ---- cutout --------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mini(device, tmp_path_factory):
    cfg = dataclasses.replace(synth.SWIN_MINI, image_size=256)
    path = synth.write_birefnet_gguf(tmp_path_factory.mktemp("bfcut") / "birefnet_mini.gguf", cfg, seed=6)
    return vision.Model.load(path, device), path


def test_birefnet_cutout_is_the_estimator_on_the_networks_mask(mini, device):
    model, _ = mini
    B, w, h, radius = 2, 256, 256, 30
    imgs = synth.images(B, w, h, seed=21)
    rgb = dev(imgs)
    mask_dev, composed, cut = guarded(B * h * w * 4), guarded(B * h * w * 4), guarded(B * h * w * 4)
    model.segment_batch_device(rgb.ptr, B, w, h, mask_dev.ptr)
    vision.estimate_foreground_batch_device(rgb.ptr, F.rgb_u8, mask_dev.ptr, B, w, h, composed.ptr, F.rgba_u8, radius, device)
    model.birefnet_cutout_batch_device(rgb.ptr, B, w, h, cut.ptr, radius)
    masks = read_guarded(mask_dev, np.float32, (B, h, w))
    got = read_guarded(cut, np.uint8, (B, h, w, 4))
    assert np.array_equal(got, read_guarded(composed, np.uint8, (B, h, w, 4))), "cutout differs from estimator(compute_batch_device's mask)"
    assert np.array_equal(model.birefnet_cutout_batch(imgs, radius), got), "the host entry differs from the device entry"
    for b in range(B):
        want = R.estimate_foreground(imgs[b].astype(np.float32) / np.float32(255), masks[b], radius)
        check_foreground(f"cutout image {b}", got[b], F.rgba_u8, want, radius)
    assert np.array_equal(model.segment_batch(imgs), masks), "the mask path is unchanged by the cutout"


def test_cpp_header_vectors_and_cutout_at_the_callers_extent(mini, tmp_path):
    """tests/cpp/matting_check.cpp: the vision.h names with the reference's signatures reproduce the three vectors on the device; birefnet_cutout on a 200 x 150
    image (not the model's 256 x 256) returns rgba_u8 at 200 x 150."""
    _, path = mini
    exe = ROOT / "vision.cpp_amd" / "lib" / "matting_check"
    assert exe.exists(), "run __graft_entry__.build() first"
    w, h = 200, 150
    img = synth.images(1, w, h, seed=4)[0]
    (tmp_path / "img.raw").write_bytes(img.tobytes())
    r = subprocess.run([str(exe), str(path), str(tmp_path / "img.raw"), str(w), str(h), str(tmp_path / "out.raw")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "matting-check ok" in r.stdout, (r.stdout, r.stderr)
    out = np.frombuffer((tmp_path / "out.raw").read_bytes(), np.uint8)
    assert out.size == w * h * 4

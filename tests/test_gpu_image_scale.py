"""image_scale on the device (vx_image_scale behind visp_image_scale_batch_device) and Depth-Anything's any-extent entry built on it.

1. Device against the host function: byte-equal for the u8 formats, bit-equal for the f32 ones -- the kernel's design requirement.
2. Device against float64 (tests/image_scale_ref.py), f32 formats: |got - ref| <= E = 2^-23 (n_x + n_y) A_x A_y max|src| per case, n the largest tap
   count and A the largest sum of |w| of an axis as the reference returns them, max|src| over what is filtered (colour x alpha for rgba_f32).
   rgba_f32's colour is a quotient P / a of two filtered values, each within E: |P' / a' - P / a| <= (E + |c| E) / (a - E) + 2^-22 |c| (the last
   term: the reciprocal's and the product's rounding), held where the reference's alpha is at least 0.25.
3. Device against float64, u8 formats, smooth content: colour and alpha within one level; with both, colour where the reference's alpha is >= 64.
4. compute_scaled_batch_device equals the host composition image_scale -> compute_batch_device -> image_scale exactly, and compute_batch_device at
   the model's own extent. Every case scales a batch of three different images once; the three comparisons share that result."""
import functools

import numpy as np
import pytest

import image_scale_ref as ref
from visioncpp_amd import synth, vision

pytestmark = pytest.mark.gpu

TW, TH = 64, 8  # the kernel's tile (csrc/image_scale_tables.h)
FORMATS = list(ref.CHANNELS)
EXTENTS = [(1, 1, 5, 3),                    # source h, w -> target h, w, each the smallest of its kind: a source smaller than any support
           (5, 7, 70, 56),                  # taps clamp at both edges
           (20, 30, 20, 30),                # scale exactly 1 takes the reducing filter
           (33, 47, TH + 1, 2 * TW + 3),    # ragged last tile on both axes
           (64, 48, 17, 23),                # plain reduction
           (100, 37, 37, 100),              # one axis reduces while the other enlarges
           (9, 700, 4, 16),                 # ratio 44: the tile narrows (176 taps a column)
           (3, 3, 3, 200)]                  # extreme enlargement
CASES = [pytest.param(f, e, id=f"{f}-{e[0]}x{e[1]}-{e[2]}x{e[3]}") for e in EXTENTS for f in FORMATS]


def make_inputs(fmt: str, h: int, w: int) -> np.ndarray:
    """[3, h, w, ch]: three different smooth images. Formats with alpha: images 0 and 2 have alpha >= 64 levels (0.25) everywhere, image 1 holds a
    block of alpha 0 (8 x 8, at most half the extent). f32 values span [-0.5, 1.5] (alpha stays in [0, 1])."""
    ch, ac, u8 = ref.CHANNELS[fmt], ref.ALPHA[fmt], fmt.endswith("u8")
    rng = np.random.default_rng(1000 * h + w + len(fmt))
    yy, xx = np.mgrid[0:h, 0:w]
    out = np.empty((3, h, w, ch), np.float64)
    for b in range(3):
        for c in range(ch):
            wave = np.sin(xx / (3.1 + b) + c) * np.cos(yy / (4.3 - b) - c)  # in [-1, 1]
            out[b, ..., c] = 0.65 + 0.35 * wave if c == ac else 0.5 + (0.47 if u8 else 1.0) * wave
        if ac >= 0 and b == 1:
            out[b, :max(1, min(8, h // 2)), :max(1, min(8, w // 2)), ac] = 0.0
    if u8:
        return np.clip(np.rint(out * 255.0 + rng.normal(0, 2, out.shape) * (out > 0)), 0, 255).astype(np.uint8)
    return out.astype(np.float32)


@functools.lru_cache(maxsize=None)
def reference(fmt: str, ext: tuple):
    h, w, oh, ow = ext
    return ref.image_scale(make_inputs(fmt, h, w), fmt, oh, ow)


@pytest.fixture(scope="module")
def device():
    return vision.Device.init(vision.Backend.gpu)


@pytest.fixture(scope="module")
def scaled(device):
    """(fmt, ext) -> the device's result [3, oh, ow, ch], computed once, through the device-pointer entry"""
    done = {}

    def get(fmt, ext):
        if (fmt, ext) not in done:
            h, w, oh, ow = ext
            src = make_inputs(fmt, h, w)
            x, y = vision.DeviceBuffer.from_numpy(src), vision.DeviceBuffer(3 * oh * ow * src.shape[3] * src.itemsize)
            vision.image_scale_batch_device(x.ptr, vision.ImageFormat[fmt], 3, w, h, y.ptr, ow, oh, device=device)
            done[fmt, ext] = y.to_numpy(src.dtype, (3, oh, ow, src.shape[3]))
        return done[fmt, ext]

    return get


def check_f32(got: np.ndarray, fmt: str, ext: tuple):
    want, alpha, (nx, ny), (ax, ay) = reference(fmt, ext)
    src = make_inputs(fmt, ext[0], ext[1]).astype(np.float64)
    ac = ref.ALPHA[fmt]
    if fmt == "rgba_f32":
        src[..., :3] *= src[..., 3:]
    E = 2.0 ** -23 * (nx + ny) * ax * ay * np.abs(src).max()
    err = np.abs(got.astype(np.float64) - want)
    print(f"{fmt} {ext}: n {nx}+{ny} A {ax:.3f} x {ay:.3f} bound {E:.3e} largest error {err[..., ac].max() if fmt == 'rgba_f32' else err.max():.3e}")
    if fmt != "rgba_f32":
        assert err.max() <= E, (err.max(), E)
        return
    assert err[..., 3].max() <= E, (err[..., 3].max(), E)
    held = alpha >= 0.25
    c = np.abs(want[..., :3][held])
    bound = (E + c * E) / (alpha[held][:, None] - E) + 2.0 ** -22 * c
    assert (err[..., :3][held] <= bound).all(), float((err[..., :3][held] / bound).max())


def check_u8(got: np.ndarray, fmt: str, ext: tuple):
    want, alpha, _, _ = reference(fmt, ext)
    ch, ac = ref.CHANNELS[fmt], ref.ALPHA[fmt]
    d = np.abs(got.astype(np.float64) - np.rint(want))
    if ac >= 0:
        assert d[..., ac].max() <= 1, ("alpha", d[..., ac].max())
    if ch > 1:
        colour = [c for c in range(ch) if c != ac]
        dc = d[..., colour] if ac < 0 else d[..., colour][alpha * 255.0 >= 64]
        print(f"{fmt} {ext}: colour levels off: largest {dc.max() if dc.size else 0:.0f} mean {dc.mean() if dc.size else 0:.4f}")
        assert dc.size == 0 or dc.max() <= 1, ("colour", dc.max())


@pytest.mark.parametrize("fmt, ext", CASES)
def test_device_equals_the_host_function(scaled, fmt, ext):
    h, w, oh, ow = ext
    src, got = make_inputs(fmt, h, w), scaled(fmt, ext)
    host = np.stack([vision.image_scale(src[b], ow, oh, vision.ImageFormat[fmt]).reshape(oh, ow, -1) for b in range(3)])
    if fmt.endswith("u8"):
        assert np.array_equal(got, host), int((got != host).sum())
    else:
        assert np.array_equal(got.view(np.uint32), host.view(np.uint32)), int((got.view(np.uint32) != host.view(np.uint32)).sum())


@pytest.mark.parametrize("fmt, ext", [c for c in CASES if c.values[0].endswith("f32")])
def test_f32_formats_against_float64(scaled, fmt, ext):
    check_f32(scaled(fmt, ext), fmt, ext)


@pytest.mark.parametrize("fmt, ext", [c for c in CASES if c.values[0].endswith("u8")])
def test_u8_formats_against_float64(scaled, fmt, ext):
    check_u8(scaled(fmt, ext), fmt, ext)


def test_numpy_entry_on_the_device(device):
    src = make_inputs("rgb_u8", 33, 47)
    got = vision.image_scale(src, 60, 21, vision.ImageFormat.rgb_u8, device=device)
    assert np.array_equal(got, np.stack([vision.image_scale(s, 60, 21) for s in src]))


@pytest.fixture(scope="module")
def mini(device, tmp_path_factory):
    return vision.Model.load(synth.write_gguf(tmp_path_factory.mktemp("scale") / "mini.gguf", synth.MINI, seed=4), device)


@pytest.mark.parametrize("h, w", [(40, 52), (90, 70)])
def test_compute_scaled_batch_device_is_the_host_composition(mini, h, w):
    imgs = synth.images(2, w, h, seed=3)
    mw, mh = mini.image_extent(w, h)
    assert (mw, mh) != (w, h)
    x, y = vision.DeviceBuffer.from_numpy(imgs), vision.DeviceBuffer(2 * h * w * 4)
    mini.compute_scaled_batch_device(x.ptr, 2, w, h, y.ptr)
    got = y.to_numpy(np.float32, (2, h, w))
    at_model = np.stack([vision.image_scale(i, mw, mh) for i in imgs])
    xm, ym = vision.DeviceBuffer.from_numpy(at_model), vision.DeviceBuffer(2 * mh * mw * 4)
    mini.compute_batch_device(xm.ptr, 2, mw, mh, ym.ptr)
    depth = ym.to_numpy(np.float32, (2, mh, mw))
    want = np.stack([vision.image_scale(d, w, h, vision.ImageFormat.alpha_f32) for d in depth])
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(mini.compute_scaled_batch(imgs).view(np.uint32), want.view(np.uint32))  # the host twin


def test_compute_scaled_batch_device_at_the_models_extent(mini):
    w, h = mini.image_extent(112, 112)
    imgs = synth.images(2, w, h, seed=5)
    x, y, z = vision.DeviceBuffer.from_numpy(imgs), vision.DeviceBuffer(2 * h * w * 4), vision.DeviceBuffer(2 * h * w * 4)
    mini.compute_scaled_batch_device(x.ptr, 2, w, h, y.ptr)
    mini.compute_batch_device(x.ptr, 2, w, h, z.ptr)
    assert np.array_equal(y.to_numpy(np.uint32, (2, h, w)), z.to_numpy(np.uint32, (2, h, w)))

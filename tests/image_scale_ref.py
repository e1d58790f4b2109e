"""image_scale in float64 numpy, written from the filter's definition and independent of csrc/image_resize.cpp's axis_taps: a dense weight matrix
per axis, sRGB decode, premultiply, the two products, the divide. No rounding to the output type: the caller compares levels or floats."""
import numpy as np

CHANNELS = {"rgba_u8": 4, "bgra_u8": 4, "argb_u8": 4, "rgb_u8": 3, "alpha_u8": 1, "rgba_f32": 4, "rgb_f32": 3, "alpha_f32": 1}
ALPHA = {"rgba_u8": 3, "bgra_u8": 3, "argb_u8": 0, "rgb_u8": -1, "alpha_u8": 0, "rgba_f32": 3, "rgb_f32": -1, "alpha_f32": 0}


def catmull_rom(x):
    x = np.abs(x)
    return np.where(x < 1, 1 - x * x * (2.5 - 1.5 * x), np.where(x < 2, 2 - x * (4 + x * (0.5 * x - 2.5)), 0.0))


def mitchell(x):
    x = np.abs(x)
    return np.where(x < 1, (16 + x * x * (21 * x - 36)) / 18, np.where(x < 2, (32 + x * (-60 + x * (36 - 7 * x))) / 18, 0.0))


def axis_matrix(n_in: int, n_out: int):
    """(W [n_out, n_in] with rows summing to 1, the largest number of source positions inside a support, the largest sum of |w| of a row).
    Enlarging: Catmull-Rom at (i + 0.5) / scale - (n + 0.5); reducing or scale 1: Mitchell at (i + 0.5) - (n + 0.5) scale. Every integer n inside
    the support counts, those beyond the image folded onto the clamped index."""
    scale = n_out / n_in
    reach = int(np.ceil(2 / min(scale, 1.0))) + 2
    W, taps, mass = np.zeros((n_out, n_in)), 0, 0.0
    for i in range(n_out):
        n = np.arange(int(np.floor((i + 0.5) / scale)) - reach, int(np.floor((i + 0.5) / scale)) + reach + 1)
        k = catmull_rom((i + 0.5) / scale - (n + 0.5)) if scale > 1 else mitchell((i + 0.5) - (n + 0.5) * scale)
        inside = (np.abs((i + 0.5) / scale - (n + 0.5)) < 2) if scale > 1 else (np.abs((i + 0.5) - (n + 0.5) * scale) < 2)
        k = k / k.sum()
        np.add.at(W[i], np.clip(n, 0, n_in - 1), k)
        taps, mass = max(taps, int(inside.sum())), max(mass, float(np.abs(k).sum()))
    return W, taps, mass


def srgb_to_linear(u8):
    c = np.asarray(u8, np.float64) / 255.0
    return np.where(c <= 0.04045, c / 12.92, ((c + 0.055) / 1.055) ** 2.4)


def linear_to_srgb_levels(v):
    v = np.clip(v, 0.0, 1.0)
    return np.where(v <= 0.0031308, v * 12.92, 1.055 * v ** (1 / 2.4) - 0.055) * 255.0


def image_scale(images: np.ndarray, fmt: str, oh: int, ow: int):
    """images [B, h, w, ch] (u8 or f32) -> (out float64 [B, oh, ow, ch]: sRGB / alpha LEVELS for u8 formats, values for f32; alpha float64 [B, oh, ow] in
    [0, 1] units or None; n = (taps_x, taps_y); A = (mass_x, mass_y))."""
    ch, ac, u8 = CHANNELS[fmt], ALPHA[fmt], fmt.endswith("u8")
    x = np.asarray(images)
    Wy, ny, Ay = axis_matrix(x.shape[1], oh)
    Wx, nx, Ax = axis_matrix(x.shape[2], ow)
    lin = np.empty(x.shape, np.float64)
    for c in range(ch):
        lin[..., c] = (x[..., c] / 255.0 if c == ac else srgb_to_linear(x[..., c])) if u8 else x[..., c]
    if ac >= 0 and ch > 1:
        colour = [c for c in range(ch) if c != ac]
        lin[..., colour] *= lin[..., ac:ac + 1]
    out = np.einsum("yh,bhxc->byxc", Wy, np.einsum("xw,bhwc->bhxc", Wx, lin))
    alpha = out[..., ac].copy() if ac >= 0 else None
    if ac >= 0 and ch > 1:
        with np.errstate(divide="ignore", invalid="ignore"):
            out[..., colour] = np.where(alpha[..., None] != 0, out[..., colour] / alpha[..., None], 0.0)
    if u8:
        for c in range(ch):
            out[..., c] = np.clip(out[..., c], 0, 1) * 255.0 if c == ac else linear_to_srgb_levels(out[..., c])
    return out, alpha, (nx, ny), (Ax, Ay)

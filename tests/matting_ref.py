"""The matting image ops restated in numpy (reference src/visp/image.cpp:290-323, 358-535, src/visp/image-impl.h:17-41): box blur, erosion, the
blur-fusion foreground estimator, the u8 alpha composite, image_set_alpha, image_to_mask.

Two modes of the blur. `box_blur` is the definition in float64: the mean of the clamped window, every output on its own. `box_blur_running_f32`
repeats the reference's arithmetic: ONE float32 running sum along a whole row (column), the entering pixel added and the leaving one subtracted,
so that an output's error depends on everything the sum has passed. The second mode documents how far the reference sits from the definition
(DESIGN.md section 21); no test holds the kernels to it."""
import numpy as np

CHANNEL_MAP = {"rgba_u8": (0, 1, 2, 3), "bgra_u8": (2, 1, 0, 3), "argb_u8": (1, 2, 3, 0)}  # image.cpp get_channel_map


def _window_sum(x, radius, axis):
    """Sum over the clamped window [i - r, i + r] along axis, in x's dtype, by direct summation (no running sum)."""
    n = x.shape[axis]
    idx = np.clip(np.arange(n)[:, None] + np.arange(-radius, radius + 1)[None, :], 0, n - 1)  # [n, 2r + 1]
    return np.take(x, idx, axis=axis).sum(axis=axis + 1)


def check_radius(radius, w, h):
    if radius < 1 or radius > w // 2 or radius > h // 2:
        raise ValueError(f"radius {radius} is not legal for {w}x{h}")


def box_blur(x, radius):
    """x [h, w] or [h, w, c] -> float64: horizontal pass, then vertical pass, weight 1 / (2 r + 1), edges replicated."""
    x = np.asarray(x, np.float64)
    check_radius(radius, x.shape[1], x.shape[0])
    return _window_sum(_window_sum(x, radius, 1), radius, 0) / float(2 * radius + 1) ** 2


def box_blur_running_f32(x, radius):
    """The reference's blur<T> step for step in float32 (image.cpp:358-408)."""
    x = np.asarray(x, np.float32)
    check_radius(radius, x.shape[1], x.shape[0])
    weight = np.float32(1.0) / np.float32(2 * radius + 1)

    def one_pass(src):  # along axis 1
        n = src.shape[1]
        out = np.empty_like(src)
        s = np.float32(radius) * src[:, 0]
        for i in range(radius + 1):
            s = s + src[:, i]
        out[:, 0] = s * weight
        for i in range(1, n):
            s = s - src[:, min(max(i - radius - 1, 0), n - 1)]
            s = s + src[:, min(max(i + radius, 0), n - 1)]
            out[:, i] = s * weight
        return out

    t = one_pass(x)
    return np.swapaxes(one_pass(np.ascontiguousarray(np.swapaxes(t, 0, 1))), 0, 1)


def erosion(x, radius):
    """Minimum over the clamped (2 r + 1)^2 neighbourhood and the format's one (255 / 1.0), in x's dtype: exact."""
    x = np.asarray(x)
    one = x.dtype.type(255 if x.dtype == np.uint8 else 1.0)
    h, w = x.shape
    ys = np.clip(np.arange(h)[:, None] + np.arange(-radius, radius + 1)[None, :], 0, h - 1)
    xs = np.clip(np.arange(w)[:, None] + np.arange(-radius, radius + 1)[None, :], 0, w - 1)
    rows = x[:, xs].min(axis=2)      # [h, w]
    return np.minimum(rows[ys, :].min(axis=1), one)


def _stage(img, fg, bg, m, radius):
    m3 = m[..., None]
    bm = box_blur(m, radius)[..., None]
    bf = box_blur(fg * m3, radius) / (bm + 1e-5)
    bb = box_blur(bg * (1.0 - m3), radius) / (1.0 - bm + 1e-5)
    f = np.clip(bf + m3 * (img - m3 * bf - (1.0 - m3) * bb), 0.0, 1.0)
    return f, bb


def estimate_foreground(img_rgb, mask, radius=30):
    """img_rgb [h, w, 3] in [0, 1], mask [h, w] -> float64 [h, w, 4]: two blur-fusion stages (radius, then 3), alpha = clamp(mask, 0, 1)."""
    img = np.asarray(img_rgb, np.float64)
    m = np.asarray(mask, np.float64)
    f1, b1 = _stage(img, img, img, m, radius)
    f2, _ = _stage(img, f1, b1, m, 3)
    return np.concatenate([f2, np.clip(m, 0.0, 1.0)[..., None]], axis=2)


def store_u8(v):
    """image_store (image-impl.h:34-41): uint8(clamp(v, 0, 1) * 255), truncating, in float32."""
    return (np.clip(np.asarray(v, np.float32), np.float32(0), np.float32(1)) * np.float32(255)).astype(np.uint8)


def alpha_composite(fg_rgba, bg, mask):
    """The reference's float32 arithmetic on u8 images (image.cpp:478-489): every product and sum rounded on its own, truncating store."""
    f32 = np.float32
    w = (np.asarray(mask, np.uint8).astype(f32) / f32(255))[..., None]
    fg = np.asarray(fg_rgba, np.uint8)[..., :3].astype(f32) / f32(255)
    b = np.asarray(bg, np.uint8)[..., :3].astype(f32) / f32(255)
    v = w * fg + (f32(1) - w) * b
    out = np.empty(fg.shape[:2] + (4,), np.uint8)
    out[..., :3] = store_u8(v)
    out[..., 3] = 255
    return out


def set_alpha(img, alpha, fmt="rgba_u8"):
    out = np.array(img, np.uint8, copy=True)
    out[..., CHANNEL_MAP[fmt][3]] = alpha
    return out


def to_mask(img):
    img = np.asarray(img, np.uint8)
    return img if img.ndim == 2 else img[..., 0].copy()

"""MI-GAN oracle in numpy (reference src/visp/arch/migan.cpp, src/visp/vision.cpp:172-203), composed only of the CPU
oracle's primitives (oracle/oracle.py: conv2d_nhwc, conv2d_depthwise_nhwc, image_scale, image_f32_to_u8). Weights are a
state dict with torch names and shapes (visioncpp_amd.synth.migan_state_dict), f32; round them through f16 to compare with
a GGUF file."""
from __future__ import annotations

import numpy as np

from oracle import oracle

SQRT2 = np.float32(np.sqrt(2.0))


def lrelu_agc(x: np.ndarray) -> np.ndarray:
    """migan.cpp:17-26 with alpha 0.2, gain sqrt2, clamp 256."""
    x = np.where(x < 0, np.float32(0.2) * x, x).astype(np.float32)
    return np.clip(x * SQRT2, -256.0, 256.0).astype(np.float32)


def depthwise(x: np.ndarray, w: np.ndarray, b: np.ndarray | None, stride: int, pad: int) -> np.ndarray:
    """x [B,H,W,C], w torch [C,1,k,k]."""
    wk = np.ascontiguousarray(w[:, 0].transpose(1, 2, 0))
    return np.stack([oracle.conv2d_depthwise_nhwc(x[i], wk, b, stride, pad) for i in range(x.shape[0])])


def conv1x1(x: np.ndarray, w: np.ndarray, b: np.ndarray | None = None) -> np.ndarray:
    """x [B,H,W,Cin], w torch [Cout,Cin,1,1]."""
    return oracle.conv2d_nhwc(x, np.ascontiguousarray(w.transpose(0, 2, 3, 1)), b)


def downsample(x: np.ndarray, f: np.ndarray) -> np.ndarray:
    """migan.cpp:28-30: depthwise 4x4, stride 2, pad 1."""
    return depthwise(x, f, None, 2, 1)


def upsample(x: np.ndarray, f: np.ndarray, filter_const: np.ndarray | None = None) -> np.ndarray:
    """migan.cpp:32-51: nearest x2, times filter_const, depthwise 4x4 with pad 2, last row / column dropped."""
    B, h, w, C = x.shape
    up = np.repeat(np.repeat(x, 2, axis=1), 2, axis=2)
    fc = filter_const.reshape(2 * h, 2 * w) if filter_const is not None else np.tile(np.array([[1, 0], [0, 0]], np.float32), (h, w))
    up = (up * fc[None, :, :, None]).astype(np.float32)
    return depthwise(up, f, None, 1, 2)[:, :2 * h, :2 * w]


def separable_conv(sd: dict, p: str, x: np.ndarray, down=False, up=False, noise=False) -> np.ndarray:
    """migan.cpp:53-82 with the activation (every separable conv of the generator has it)."""
    x = lrelu_agc(depthwise(x, sd[f"{p}.conv1.weight"], sd[f"{p}.conv1.bias"], 1, 1))
    if down:
        x = downsample(x, sd[f"{p}.downsample.filter.weight"])
    x = conv1x1(x, sd[f"{p}.conv2.weight"])
    if up:
        x = upsample(x, sd[f"{p}.upsample.filter.weight"], sd[f"{p}.upsample.filter_const"])
    if noise:
        x = x + (sd[f"{p}.noise_const"] * sd[f"{p}.noise_strength"].reshape(())).astype(np.float32)[None, :, :, None]
    return lrelu_agc(x)


def levels(res: int) -> list[int]:
    out, r = [], res
    while r >= 4:
        out.append(r)
        r //= 2
    return out


def encode(sd: dict, x4: np.ndarray, res: int):
    """migan.cpp:84-114: returns (x at 4 x 4, {r: skip feature})."""
    x = lrelu_agc(conv1x1(x4, sd[f"encoder.b{res}.fromrgb.weight"], sd[f"encoder.b{res}.fromrgb.bias"]))
    feats = {}
    rs = levels(res)
    for r in rs:
        p = f"encoder.b{r}"
        feats[r] = separable_conv(sd, f"{p}.conv1", x)
        x = separable_conv(sd, f"{p}.conv2", feats[r], down=r != 4)
    return x, feats


def synthesize(sd: dict, x: np.ndarray, feats: dict, res: int, captures: dict | None = None):
    """migan.cpp:116-140: rgb f32 [B,res,res,3]."""
    img = None
    for r in reversed(levels(res)):
        p = f"synthesis.b{r}"
        first = r == 4
        x = separable_conv(sd, f"{p}.conv1", x, up=not first, noise=not first) + feats[r]
        x = separable_conv(sd, f"{p}.conv2", x, noise=not first)
        y = conv1x1(x, sd[f"{p}.torgb.weight"], sd[f"{p}.torgb.bias"])
        img = y if img is None else upsample(img, sd[f"{p}.upsample.filter.weight"], sd[f"{p}.upsample.filter_const"]) + y
        if captures is not None:
            captures[f"syn.b{r}.x"], captures[f"syn.b{r}.img"] = x, img
    return img


def generate(sd: dict, x4: np.ndarray, res: int, captures: dict | None = None) -> np.ndarray:
    x, feats = encode(sd, np.asarray(x4, np.float32), res)
    if captures is not None:
        captures.update({f"enc.feat{r}": f for r, f in feats.items()})
        captures["enc.out"] = x
    return synthesize(sd, x, feats, res, captures)


def preprocess(image: np.ndarray, mask: np.ndarray, res: int) -> np.ndarray:
    """migan_process_input (migan.cpp:142-159, 181-196) with invert_mask: u8 image [h,w,3|4] + u8 mask [h,w] -> f32 [res,res,4]."""
    fmt = oracle.RGB_U8 if image.shape[2] == 3 else oracle.RGBA_U8
    if image.shape[:2] != (res, res):
        image = oracle.image_scale(image, fmt, res, res)
    if mask.shape[:2] != (res, res):
        mask = oracle.image_scale(mask, oracle.ALPHA_U8, res, res)
    a = np.float32(1.0) - mask.astype(np.float32) / np.float32(255.0)
    rgb = image[..., :3].astype(np.float32) / np.float32(255.0)
    color = a[..., None] * (rgb * np.float32(2.0) - np.float32(1.0))
    return np.concatenate([(a - np.float32(0.5))[..., None], color], axis=-1).astype(np.float32)


def postprocess(rgb: np.ndarray, mask: np.ndarray) -> np.ndarray:
    """migan_process_output (migan.cpp:198-206) + image_set_alpha with the original mask: rgb f32 [res,res,3] -> rgba u8 at the
    mask's extent."""
    h, w = mask.shape[:2]
    if rgb.shape[:2] != (h, w):
        rgb = oracle.image_scale(np.ascontiguousarray(rgb, np.float32), oracle.RGB_F32, w, h)
    out = oracle.image_f32_to_u8(rgb, oracle.RGB_F32, oracle.RGBA_U8, 0.5, 0.5)
    out[..., 3] = mask
    return out


def compute(sd: dict, res: int, image: np.ndarray, mask: np.ndarray) -> np.ndarray:
    """migan_compute (vision.cpp:172-203): any extent in, rgba u8 at that extent out."""
    x4 = preprocess(image, mask, res)
    rgb = generate(sd, x4[None], res)[0]
    return postprocess(rgb, mask)


def f16_rounded(sd: dict) -> dict:
    return {k: v.astype(np.float16).astype(np.float32) for k, v in sd.items()}

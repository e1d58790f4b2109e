"""numpy restatement of the reference's YOLOv9t (src/visp/arch/yolov9t.cpp) on the CPU oracle's primitives (oracle/oracle.py:
conv2d_nhwc, image_scale): the network on NHWC f32 maps, the detect head's decode, letterbox, non_max_suppression and scale_boxes.
Weights are the folded tensor set (vision.cpp_amd/convert.py fold_yolov9t): name -> float32 torch-layout array. RepConv is evaluated
as the reference does it, two convs added (the backend folds the 1x1 into the 3x3)."""
from __future__ import annotations

import math
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from oracle import oracle  # noqa: E402

REP_N = 3


def f16_rounded(sd: dict[str, np.ndarray]) -> dict[str, np.ndarray]:
    """What the GGUF holds: conv kernels rounded to f16, biases f32."""
    return {k: (v.astype(np.float16).astype(np.float32) if v.ndim == 4 else v.astype(np.float32)) for k, v in sd.items()}


def silu(x):
    return x / (1.0 + np.exp(-x))


def conv(W, name, x, stride=1, act=True):
    """Conv (yolov9t.cpp:78-120): conv_2d with autopad k // 2 + bias, then SiLU (BatchNorm folded). `name` without ".weight"."""
    w, b = W[name + ".weight"], W[name + ".bias"]
    y = oracle.conv2d_nhwc(x, np.ascontiguousarray(w.transpose(0, 2, 3, 1)), b, stride, w.shape[2] // 2)
    return silu(y) if act else y


def repconv(W, p, x):  # yolov9t.cpp:256-302: conv1 3x3 + conv2 1x1 (no act each), added, SiLU
    return silu(conv(W, p + ".conv1.conv", x, act=False) + conv(W, p + ".conv2.conv", x, act=False))


def avg_pool2(x):  # ggml_pool_2d AVG 2x2 / s1 / p0 (yolov9t.cpp:165-185)
    return (x[:, :-1, :-1] + x[:, 1:, :-1] + x[:, :-1, 1:] + x[:, 1:, 1:]) * 0.25


def max_pool5(x):  # ggml_pool_2d MAX 5x5 / s1 / p2, padded positions never win (yolov9t.cpp:458-463)
    B, H, W, C = x.shape
    p = np.full((B, H + 4, W + 4, C), -np.inf, np.float32)
    p[:, 2:-2, 2:-2] = x
    return np.max(np.stack([p[:, dy:dy + H, dx:dx + W] for dy in range(5) for dx in range(5)]), axis=0)


def upsample2(x):  # nearest x2 (yolov9t.cpp:486-493)
    return x.repeat(2, axis=1).repeat(2, axis=2)


def aconv(W, p, x):  # yolov9t.cpp:165-185
    return conv(W, p + ".cv1.conv", avg_pool2(x), stride=2)


def elan1(W, p, x):  # yolov9t.cpp:187-240: concat [cv1 out (both halves), cv2, cv3]
    a = conv(W, p + ".cv1.conv", x)
    c2 = conv(W, p + ".cv2.conv", a[..., a.shape[-1] // 2:])
    c3 = conv(W, p + ".cv3.conv", c2)
    return conv(W, p + ".cv4.conv", np.concatenate([a, c2, c3], -1))


def repcsp(W, p, x):  # yolov9t.cpp:370-404 with RepBottleneck :304-330 (shortcut, c1 == c2)
    m = conv(W, p + ".cv1.conv", x)
    y2 = conv(W, p + ".cv2.conv", x)
    for j in range(REP_N):
        q = f"{p}.m.{j}"
        m = m + conv(W, q + ".cv2.conv", repconv(W, q + ".cv1", m))
    return conv(W, p + ".cv3.conv", np.concatenate([m, y2], -1))


def repncspelan4(W, p, x):  # yolov9t.cpp:406-447: concat [cv1 out (all c3), cv2, cv3]
    a = conv(W, p + ".cv1.conv", x)
    c2 = conv(W, p + ".cv2.1.conv", repcsp(W, p + ".cv2.0", a[..., a.shape[-1] // 2:]))
    c3 = conv(W, p + ".cv3.1.conv", repcsp(W, p + ".cv3.0", c2))
    return conv(W, p + ".cv4.conv", np.concatenate([a, c2, c3], -1))


def sppelan(W, p, x):  # yolov9t.cpp:449-484
    c1 = conv(W, p + ".cv1.conv", x)
    c2 = max_pool5(c1)
    c3 = max_pool5(c2)
    c4 = max_pool5(c3)
    return conv(W, p + ".cv5.conv", np.concatenate([c1, c2, c3, c4], -1))


def backbone(W, x):
    """yolov9t_backbone (yolov9t.cpp:507-630): x f32 [B, S, S, 3] -> {i: feature map} for i = 0..21."""
    f = {}
    f[0] = conv(W, "model.0.conv", x, 2)
    f[1] = conv(W, "model.1.conv", f[0], 2)
    f[2] = elan1(W, "model.2", f[1])
    f[3] = aconv(W, "model.3", f[2])
    f[4] = repncspelan4(W, "model.4", f[3])
    f[5] = aconv(W, "model.5", f[4])
    f[6] = repncspelan4(W, "model.6", f[5])
    f[7] = aconv(W, "model.7", f[6])
    f[8] = repncspelan4(W, "model.8", f[7])
    f[9] = sppelan(W, "model.9", f[8])
    f[10] = upsample2(f[9])
    f[11] = np.concatenate([f[10], f[6]], -1)
    f[12] = repncspelan4(W, "model.12", f[11])
    f[13] = upsample2(f[12])
    f[14] = np.concatenate([f[13], f[4]], -1)
    f[15] = repncspelan4(W, "model.15", f[14])
    f[16] = aconv(W, "model.16", f[15])
    f[17] = np.concatenate([f[16], f[12]], -1)
    f[18] = repncspelan4(W, "model.18", f[17])
    f[19] = aconv(W, "model.19", f[18])
    f[20] = np.concatenate([f[19], f[9]], -1)
    f[21] = repncspelan4(W, "model.21", f[20])
    return f


def head_raw(W, feats):
    """detect_forward's convs (yolov9t.cpp:770-800): per level concat [cv2 box branch (64), cv3 class branch (nc)]."""
    out = []
    for lv, x in enumerate(feats):
        r = conv(W, f"detect.cv2.{lv}.0.conv", x)
        r = conv(W, f"detect.cv2.{lv}.1.conv", r)
        r = conv(W, f"detect.cv2.{lv}.2", r, act=False)
        c = conv(W, f"detect.cv3.{lv}.0.conv", x)
        c = conv(W, f"detect.cv3.{lv}.1.conv", c)
        c = conv(W, f"detect.cv3.{lv}.2", c, act=False)
        out.append(np.concatenate([r, c], -1))
    return out


def decode(raws):
    """inference (yolov9t.cpp:693-768): dfl_forward (:657-691), make_anchors (:875-925, cell + 0.5, y-major, levels 8/16/32),
    dist2bbox xyxy (:631-655) times the stride; sigmoid of the class logits. -> boxes [B, A, 4], scores [B, A, nc] (float32)."""
    boxes, scores = [], []
    for lv, r in enumerate(raws):
        B, h, w, ch = r.shape
        stride = 8.0 * 2 ** lv
        r = r.reshape(B, h * w, ch).astype(np.float64)
        logits = r[..., :64].reshape(B, h * w, 4, 16)
        e = np.exp(logits - logits.max(-1, keepdims=True))
        d = (e * np.arange(16)).sum(-1) / e.sum(-1)
        gy, gx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
        anc = np.stack([gx.ravel() + 0.5, gy.ravel() + 0.5], -1)[None]
        boxes.append(np.concatenate([anc - d[..., :2], anc + d[..., 2:]], -1) * stride)
        scores.append(1.0 / (1.0 + np.exp(-r[..., 64:])))
    return np.concatenate(boxes, 1).astype(np.float32), np.concatenate(scores, 1).astype(np.float32)


def forward(W, x, return_features=False):
    f = backbone(W, np.asarray(x, np.float32))
    raws = head_raw(W, [f[15], f[18], f[21]])
    boxes, scores = decode(raws)
    return (boxes, scores, f, raws) if return_features else (boxes, scores)


# ---- host pre / post processing -------------------------------------------------------------------------------------------

def _round_half_away(v) -> int:  # std::round of a non-negative float
    return int(math.floor(float(v) + 0.5))


def letterbox(image: np.ndarray, size: int = 640):
    """letterbox (yolov9t.cpp:1028-1083) with _auto = scaleFill = false, scaleup = true, colour 114; rgba inputs lose alpha first.
    -> (rgb u8 [size, size, 3], gain, pad_w, pad_h)"""
    rgb = np.ascontiguousarray(image[..., :3], np.uint8)
    h, w = rgb.shape[:2]
    r = min(np.float32(size) / np.float32(h), np.float32(size) / np.float32(w))
    nw, nh = _round_half_away(np.float32(w) * r), _round_half_away(np.float32(h) * r)
    dw, dh = np.float32(size - nw) / np.float32(2), np.float32(size - nh) / np.float32(2)
    scaled = oracle.image_scale(rgb, oracle.RGB_U8, nw, nh)
    left, top = _round_half_away(dw - np.float32(0.1)), _round_half_away(dh - np.float32(0.1))
    out = np.full((size, size, 3), 114, np.uint8)
    out[top:top + nh, left:left + nw] = scaled
    return out, float(r), float(dw), float(dh)


DEFAULTS = dict(conf=0.25, iou=0.45, max_det=300, max_nms=30000, max_wh=640)


def _box_iou(b1, b2):  # yolov9t.cpp:1100-1115 in float32
    f = np.float32
    ix1, iy1, ix2, iy2 = max(b1[0], b2[0]), max(b1[1], b2[1]), min(b1[2], b2[2]), min(b1[3], b2[3])
    iw, ih = max(f(0), f(ix2 - ix1)), max(f(0), f(iy2 - iy1))
    inter = f(iw * ih)
    a1 = f(f(b1[2] - b1[0]) * f(b1[3] - b1[1]))
    a2 = f(f(b2[2] - b2[0]) * f(b2[3] - b2[1]))
    u = f(f(a1 + a2) - inter)
    return f(inter / u) if u > 0 else f(0)


def nms(boxes: np.ndarray, scores: np.ndarray, conf=0.25, iou=0.45, max_det=300, max_nms=30000, max_wh=640):
    """non_max_suppression (yolov9t.cpp:1145-1253) + nms (:1117-1143): multi-label candidates with score >= conf, the best max_nms,
    greedy suppression with the class offset on x only, max_det kept. Score ties in (anchor, class) order.
    -> list of (x1, y1, x2, y2, score, class) with float32 values."""
    boxes = np.asarray(boxes, np.float32)
    scores = np.asarray(scores, np.float32)
    A, nc = scores.shape
    a_idx, c_idx = np.nonzero(scores >= np.float32(conf))
    s = scores[a_idx, c_idx]
    order = np.lexsort((c_idx, a_idx, -s.astype(np.float64)))[:max_nms]
    a_idx, c_idx, s = a_idx[order], c_idx[order], s[order]
    f = np.float32
    removed = np.zeros(len(s), bool)
    out = []
    for i in range(len(s)):
        if len(out) >= max_det:
            break
        if removed[i]:
            continue
        bi = boxes[a_idx[i]]
        oi = f(int(c_idx[i]) * max_wh)
        b1 = (f(bi[0] + oi), bi[1], f(bi[2] + oi), bi[3])
        out.append((bi[0], bi[1], bi[2], bi[3], s[i], int(c_idx[i])))
        for j in range(i + 1, len(s)):
            if removed[j]:
                continue
            bj = boxes[a_idx[j]]
            oj = f(int(c_idx[j]) * max_wh)
            b2 = (f(bj[0] + oj), bj[1], f(bj[2] + oj), bj[3])
            if _box_iou(b1, b2) > f(iou):
                removed[j] = True
    return out


def scale_boxes(dets, w: int, h: int, gain: float, pad_w: float, pad_h: float):
    """scale_boxes (yolov9t.cpp:1255-1281): (v - pad) / gain with the unrounded pads, clamped to the image."""
    f = np.float32
    g, pw, ph = f(gain), f(pad_w), f(pad_h)
    out = []
    for x1, y1, x2, y2, s, c in dets:
        out.append((min(max(f((x1 - pw) / g), f(0)), f(w)), min(max(f((y1 - ph) / g), f(0)), f(h)),
                    min(max(f((x2 - pw) / g), f(0)), f(w)), min(max(f((y2 - ph) / g), f(0)), f(h)), s, c))
    return out


def detect(W, image: np.ndarray, size: int = 640, **kw):
    """inference_yolov9t.cpp:300-405: letterbox, u8 / 255, network, NMS, scale_boxes."""
    img, gain, pw, ph = letterbox(image, size)
    boxes, scores = forward(W, (img.astype(np.float32) / np.float32(255))[None])
    return scale_boxes(nms(boxes[0], scores[0], **kw), image.shape[1], image.shape[0], gain, pw, ph), boxes[0], scores[0]

"""The way back from COCO's uncompressed RLE and the pairwise IoU of masks, as the definitions read: plain loops and numpy integer sums. Decode is
vision.rle_to_mask's loop with the clamp of a row that is short (pixels behind its last run are background) or long (runs and parts of runs behind h w are
ignored). Integers are compared by equality; the one division is float64."""
import numpy as np


def decode(counts, w: int, h: int):
    """-> (mask bool [h, w], area = foreground pixels written, status: 0 the runs sum to h w, 1 short, 2 long)"""
    flat = np.zeros(h * w, bool)
    pos, value = 0, False
    for c in counts:
        flat[min(pos, h * w):min(pos + c, h * w)] = value
        pos += c
        value = not value
    return flat.reshape(w, h).T, int(flat.sum()), 0 if pos == h * w else 1 if pos < h * w else 2


def csr(rows):
    """lists of counts -> (offsets i64 [n + 1], runs u32): the rows one behind the other"""
    offsets = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    return offsets, np.concatenate([np.asarray(r, np.uint32) for r in rows])


def iou(a, b, iscrowd=None):
    """a bool [na, h, w], b bool [nb, h, w] -> (inter i64 [na, nb], den i64 [na, nb], iou f64 [na, nb]): COCO's rule, den = the union, or a's area where
    iscrowd[j]; iou 0 where den is 0"""
    a, b = np.asarray(a, bool), np.asarray(b, bool)
    inter = np.array([[int((x & y).sum()) for y in b] for x in a], np.int64)
    area_a, area_b = a.sum((1, 2), dtype=np.int64), b.sum((1, 2), dtype=np.int64)
    den = area_a[:, None] + area_b[None, :] - inter
    if iscrowd is not None:
        den = np.where(np.asarray(iscrowd, bool)[None, :], area_a[:, None], den)
    return inter, den, np.where(den > 0, inter.astype(np.float64) / np.maximum(den, 1), 0.0)

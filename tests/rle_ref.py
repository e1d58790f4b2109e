"""COCO's uncompressed RLE as SAM's mask_to_rle_pytorch writes it, as the definition reads: the pixels in column-major order, a boundary wherever a pixel
differs from the one before it (background before the first), the runs between the boundaries. Integers only: every comparison against it is equality."""
import numpy as np


def mask_to_rle(mask: np.ndarray) -> dict:
    """mask [h, w], non-zero = foreground -> {"size": [h, w], "counts": [...]}"""
    h, w = mask.shape
    bits = np.asarray(mask != 0).T.ravel()  # p = x * h + y
    counts, last, before = [], 0, False
    for p in range(h * w):
        if bits[p] != before:
            counts.append(p - last)
            last, before = p, bits[p]
    counts.append(h * w - last)
    return {"size": [h, w], "counts": counts}


"""The mask contents the RLE tests share; tests/rle_ref.py, the definition, knows nothing of them."""
import numpy as np


def named_masks(w: int, h: int) -> dict:
    """the contents of the kernel test at one extent: {name: u8 [h, w]}"""
    yy, xx = np.mgrid[0:h, 0:w]
    p = xx * h + yy
    rng = np.random.default_rng(w * 1000 + h)
    edges = np.zeros((h, w), np.uint8)
    edges[0], edges[-1] = 255, 255
    return {
        "zero": np.zeros((h, w), np.uint8), "full": np.full((h, w), 255, np.uint8), "first": np.where(p == 0, 255, 0).astype(np.uint8),
        "last": np.where(p == h * w - 1, 255, 0).astype(np.uint8), "checker": np.where(p % 2 == 0, 255, 0).astype(np.uint8), "edges": edges,
        "disc": np.where((xx - w / 2) ** 2 * h * h + (yy - h / 2) ** 2 * w * w <= 0.16 * w * w * h * h, 255, 0).astype(np.uint8),
        "random": rng.choice(np.array([0, 1, 128, 255], np.uint8), (h, w), p=[0.5, 1 / 6, 1 / 6, 1 / 6]),
    }

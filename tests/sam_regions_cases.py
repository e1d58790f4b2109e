"""The shared cases of the connected-component tests (tests/test_sam_regions_ref_cpu.py, tests/test_gpu_regions_kernels.py): u8 masks [n, h, w], each the
smallest that reaches its path. T is the tile edge of csrc/kernels_regions.hip."""
from __future__ import annotations

import numpy as np

T = 32
EXTENTS = [(1, 1), (17, 1), (1, 17), (T - 1, T - 1), (T, T), (T + 1, T + 1), (2 * T + 3, T + 5), (333, 517), (640, 480)]  # (w, h)


def random_mask(w, h, density, seed=0, values=(255,)):
    rng = np.random.default_rng(seed)
    m = np.zeros((h, w), np.uint8)
    on = rng.random((h, w)) < density
    m[on] = rng.choice(np.array(values, np.uint8), size=int(on.sum()))
    return m


def checkerboard(w, h):
    """one component in each mode under 8-connectivity (for w, h >= 2)"""
    y, x = np.mgrid[:h, :w]
    return np.where((x + y) % 2 == 0, 255, 0).astype(np.uint8)


def diagonal(w, h):
    """a one-pixel diagonal: it passes every tile corner on its way, so each link across a corner is a diagonal neighbour in another tile"""
    m = np.zeros((h, w), np.uint8)
    k = np.arange(min(w, h))
    m[k, k] = 255
    return m


def anti_diagonal(w, h):
    m = np.zeros((h, w), np.uint8)
    k = np.arange(min(w, h))
    m[k, w - 1 - k] = 255
    return m


def serpentine(w, h, pitch=2):
    """a one-pixel-wide path: every `pitch`-th row is full, joined to the next at alternating ends. One foreground component whose length is about
    w * h / pitch. The background between two full rows is a component of its own, (pitch - 1) * (w - 1) pixels: the joining column closes it."""
    m = np.zeros((h, w), np.uint8)
    for i, y in enumerate(range(0, h, pitch)):
        m[y] = 255
        if y + pitch < h:
            m[y:y + pitch, w - 1 if i % 2 == 0 else 0] = 255
    return m


def exact_area(min_area):
    """w = 40, h = 12: an island of exactly min_area pixels and one of min_area - 1, a hole of exactly min_area and one of min_area - 1 inside a large
    block; pieces are one-row strips so the areas are their lengths (min_area <= 16)"""
    assert 2 <= min_area <= 16
    m = np.zeros((12, 40), np.uint8)
    m[1, 1:1 + min_area] = 255
    m[3, 1:min_area] = 255
    m[5:12, 0:40] = 255
    m[7, 2:2 + min_area] = 0
    m[9, 2:1 + min_area] = 0
    return m


def two_equal_small_islands():
    """every island is small and two are the largest: the first in row-major order stays, all others go"""
    m = np.zeros((20, 70), np.uint8)
    m[2, 50:54] = 255       # 4 pixels
    m[2:4, 3:5] = 255       # 4 pixels, starts in the same row further left: its first pixel comes first, it stays
    m[10, 10:13] = 255      # 3 pixels
    m[15:17, 60:62] = 255   # 4 pixels, later
    return m


def hole_at_border():
    """small background components that touch the border (a corner, an edge), and a mask that is all foreground but them"""
    m = np.full((40, 45), 255, np.uint8)
    m[0:2, 0:2] = 0
    m[20:23, 44] = 0
    m[39, 10:14] = 0
    return m


def hole_between_islands():
    """w = 8, h = 40, for min_area 20: two islands of 16 pixels with a hole of 8 between them (a full row: with 8-connectivity for both sets a hole inside the
    image has one connected rim, so two islands can share a hole only where it spans the image), a large background and a large island below. The holes
    step joins the two into one island of 40, which stays; the islands step alone removes both."""
    m = np.zeros((40, 8), np.uint8)
    m[0:2] = 255
    m[3:5] = 255
    m[26:] = 255
    return m


def named_cases():
    """id -> (masks [n, h, w], min_area); every case runs in each mode"""
    w2, h2 = 2 * T + 3, T + 5
    cases = {}
    for w, h in EXTENTS:
        cases[f"random-{w}x{h}"] = (np.stack([random_mask(w, h, d, seed=w + h + i) for i, d in enumerate((0.3, 0.6))]), 5)
    cases["all-zero"] = (np.zeros((1, h2, w2), np.uint8), 50)
    cases["all-255"] = (np.full((1, h2, w2), 255, np.uint8), 50)
    cases["all-zero-large-min"] = (np.zeros((1, 9, 9), np.uint8), 100)   # the whole background is a small hole: it is filled (SAM has no exemption)
    cases["checkerboard"] = (checkerboard(w2, h2)[None], w2 * h2)
    cases["checkerboard-small-min"] = (checkerboard(w2, h2)[None], 7)
    cases["diagonal"] = (np.stack([diagonal(3 * T + 2, 3 * T + 2), anti_diagonal(3 * T + 2, 3 * T + 2)]), 3 * T)
    cases["diagonal-just-small"] = (np.stack([diagonal(3 * T + 2, 3 * T + 2), anti_diagonal(3 * T + 2, 3 * T + 2)]), 3 * T + 3)
    cases["serpentine-in-a-tile"] = (np.stack([serpentine(T, T), serpentine(T, T, 3)]), 400)
    cases["exact-min-area-7"] = (exact_area(7)[None], 7)
    cases["exact-min-area-16"] = (exact_area(16)[None], 16)
    cases["exact-min-area-2"] = (exact_area(2)[None], 2)
    cases["two-equal-small-islands"] = (two_equal_small_islands()[None], 9)
    cases["hole-at-border"] = (hole_at_border()[None], 5)
    cases["hole-between-islands"] = (hole_between_islands()[None], 20)
    cases["values-other-than-255"] = (random_mask(T + 9, T + 2, 0.5, seed=3, values=(1, 2, 128, 254, 255))[None], 6)
    for d in (0.05, 0.5, 0.95):
        cases[f"density-{d}"] = (np.stack([random_mask(97, 71, d, seed=int(d * 100) + i) for i in range(2)]), 12)
    return cases

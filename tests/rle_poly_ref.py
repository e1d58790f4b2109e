"""pycocotools' rleFrPoly as its loop reads, in Python floats (IEEE doubles) and ints: the reference of kernels_rle_poly.hip. `keys` are steps 1 to 3, the boundary
keys of a polygon; `runs` is step 4 as the loop writes it, `runs_by_parity` the rule the kernel uses in its place; `box` is numpy on a decoded mask."""
import math

import numpy as np


def _trunc(v: float) -> int:
    return int(v)  # a C cast: toward zero


def points(xy):
    """steps 1 and 2: the walked points (u, v) of a polygon [(X, Y), ..] in edge order"""
    x = [_trunc(5.0 * X + 0.5) for X, _ in xy]
    y = [_trunc(5.0 * Y + 0.5) for _, Y in xy]
    x.append(x[0])
    y.append(y[0])
    u, v = [], []
    for j in range(len(xy)):
        xs, xe, ys, ye = x[j], x[j + 1], y[j], y[j + 1]
        dx, dy = abs(xe - xs), abs(ys - ye)
        flip = (dx >= dy and xs > xe) or (dx < dy and ys > ye)
        if flip:
            xs, xe, ys, ye = xe, xs, ye, ys
        if dx == 0 and dy == 0:
            u.append(xs)
            v.append(ys)
            continue
        s = (ye - ys) / dx if dx >= dy else (xe - xs) / dy
        for d in range(max(dx, dy) + 1):
            t = (max(dx, dy) - d) if flip else d
            if dx >= dy:
                u.append(t + xs)
                v.append(_trunc(ys + s * t + 0.5))
            else:
                v.append(t + ys)
                u.append(_trunc(xs + s * t + 0.5))
    return u, v


def keys(xy, w: int, h: int):
    """step 3: the boundary keys, in point order"""
    u, v = points(xy)
    out = []
    for j in range(1, len(u)):
        if u[j] == u[j - 1]:
            continue
        xd = float(u[j] if u[j] < u[j - 1] else u[j] - 1)
        xd = (xd + 0.5) / 5.0 - 0.5
        if math.floor(xd) != xd or xd < 0 or xd > w - 1:
            continue
        yd = float(v[j] if v[j] < v[j - 1] else v[j - 1])
        yd = (yd + 0.5) / 5.0 - 0.5
        yd = math.ceil(min(max(yd, 0.0), float(h)))
        out.append(int(xd) * h + int(yd))
    return out


def runs(xy, w: int, h: int):
    """step 4 as the loop writes it"""
    a = sorted(keys(xy, w, h) + [h * w])
    a = [a[0]] + [q - p for p, q in zip(a, a[1:])]
    b, i = [a[0]], 1
    while i < len(a):
        if a[i] > 0:
            b.append(a[i])
            i += 1
        else:
            i += 1
            if i < len(a):
                b[-1] += a[i]
                i += 1
    return b


def runs_by_parity(xy, w: int, h: int):
    """step 4 as the kernel forms it: a sorted key survives iff its group of equal keys has an odd number of members, or it is h w; runs = differences from 0"""
    a = sorted(keys(xy, w, h) + [h * w])
    survivors = [k for k in sorted(set(a)) if a.count(k) % 2 or k == h * w]
    return [q - p for p, q in zip([0] + survivors, survivors)]


def box_polygon(b):
    x, y, bw, bh = b
    return [(x, y), (x, y + bh), (x + bw, y + bh), (x + bw, y)]


def box(mask):
    """the tight box (x, y, bw, bh) of a bool mask [h, w], zeros for an empty one"""
    ys, xs = np.nonzero(mask)
    return [0, 0, 0, 0] if not len(xs) else [int(xs.min()), int(ys.min()), int(xs.max() - xs.min() + 1), int(ys.max() - ys.min() + 1)]

"""numpy twin of fr_layer_outline (include/fr_raster.h): integer arithmetic only, written from the header's definition: the
disc weights in Python ints with math.isqrt, the grown plane as a maximum of m's over shifted copies, the shrunk plane
through the complement, then the kind and the tint (tests/layer_shadow_ref.py's, which the header says it is)."""
import functools
import math

import numpy as np

import layer_ref as lr
import layer_shadow_ref as sr

GROW, RING, INNER, SHRINK = 0, 1, 2, 3


def reach(rho):
    """R = ceil(rho / 16)"""
    return (rho + 15) // 16


def weight(rho, i, j):
    """K(i, j) in Python ints"""
    q = math.isqrt(65536 * (i * i + j * j))
    t = 16 * rho + 256 - q
    return 0 if t <= 0 else min(255, (255 * t + 128) // 256)


@functools.lru_cache(maxsize=None)
def _weights(rho):
    R = reach(rho)
    return tuple(tuple(weight(rho, i, j) for i in range(-R, R + 1)) for j in range(-R, R + 1))


def weights(rho):
    """K as a (2 R + 1, 2 R + 1) int64 array: element (j + R, i + R) is K(i, j)"""
    return np.array(_weights(rho), np.int64)


def grow(a, rho, outside):
    """G[A] on the plane of `a` grown by R on every side, where A is `a` inside its (h, w) and `outside` beyond:
    (h + 2 R, w + 2 R) int64"""
    a = np.asarray(a).astype(np.int64)
    h, w = a.shape
    R = reach(rho)
    pad = np.full((h + 4 * R, w + 4 * R), outside, np.int64)
    pad[2 * R:2 * R + h, 2 * R:2 * R + w] = a
    K = _weights(rho)
    out = np.zeros((h + 2 * R, w + 2 * R), np.int64)
    for j in range(2 * R + 1):
        for i in range(2 * R + 1):
            if K[j][i]:
                np.maximum(out, lr.m(pad[j:j + h + 2 * R, i:i + w + 2 * R], K[j][i]), out=out)
    return out


def alpha_planes(a0, rho):
    """the alpha of the four kinds on the window grown by R: a0 is (h, w) -> four (h + 2 R, w + 2 R) int64 arrays, element
    (R + v, R + u) for window coordinate (u, v)"""
    a0 = np.asarray(a0).astype(np.int64)
    h, w = a0.shape
    R = reach(rho)
    own = np.zeros((h + 2 * R, w + 2 * R), np.int64)
    own[R:R + h, R:R + w] = a0
    G = grow(a0, rho, 0)
    S = 255 - grow(255 - a0, rho, 255)
    return G, G - own, own - S, S


def outline_rect(layer, window, size, offset, rho, kind, rgba, srgb=False, planes=None):
    """the dst_h x dst_w x 4 pixels fr_layer_outline writes: layer (rows, stride, 4) u8, window = (src_x, src_y, w, h),
    size = (dst_w, dst_h), offset = (dx, dy).  planes: alpha_planes of the window, if the caller has them"""
    sx, sy, w, h = window
    dw, dh = size
    dx, dy = offset
    R = reach(rho)
    alpha = np.zeros((dh, dw), np.int64)
    if w and h and dw and dh:
        plane = (planes or alpha_planes(layer[sy:sy + h, sx:sx + w, 3], rho))[kind]   # covers u in [-R, w + R), v in [-R, h + R)
        x0, x1 = max(0, dx - R), min(dw, dx + w + R)
        y0, y1 = max(0, dy - R), min(dh, dy + h + R)
        if x0 < x1 and y0 < y1:
            alpha[y0:y1, x0:x1] = plane[y0 - dy + R:y1 - dy + R, x0 - dx + R:x1 - dx + R]
    return sr.tint(alpha, rgba, srgb)


def outline(layer, image, window, rect, offset, rho, kind, rgba, srgb=False, planes=None):
    """fr_layer_outline on the host: image (dst_rows, dst_stride, 4) with rect = (dst_x, dst_y, dst_w, dst_h) -> a new image"""
    out = np.array(image, np.uint8, copy=True)
    x, y, dw, dh = rect
    if dw and dh:
        out[y:y + dh, x:x + dw] = outline_rect(layer, window, (dw, dh), offset, rho, kind, rgba, srgb, planes)
    return out

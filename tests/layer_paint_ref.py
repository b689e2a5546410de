"""numpy / Python-int twin of fr_layer_paint (include/fr_raster.h): integer arithmetic only, written from the header's
definition.  A gradient is (kind, spread, (x0, y0, x1, y1), stops) with kind 0 linear / 1 radial, spread 0 pad / 1 repeat /
2 reflect, the geometry in 1/64 pixel and stops a list of (offset, (R, G, B, A)).  The composite and the sRGB tables are
layer_ref's (the library's host functions)."""
import math

import numpy as np

import layer_ref as lr

LINEAR, RADIAL = 0, 1
PAD, REPEAT, REFLECT = 0, 1, 2


def rdiv(n, d):
    """floor((2 n + d) / (2 d)) for d > 0 and n of either sign, in Python ints (// is floor)"""
    return (2 * n + d) // (2 * d)


def linear_coefficients(x0, y0, x1, y1):
    """(T0, TX, TY)"""
    dx, dy = x1 - x0, y1 - y0
    L2 = dx * dx + dy * dy
    return rdiv(((32 - x0) * dx + (32 - y0) * dy) << 32, L2), rdiv((64 * dx) << 32, L2), rdiv((64 * dy) << 32, L2)


def radial_coefficient(r):
    """R"""
    return rdiv(1 << 60, r)


def linear_t(coeff, X, Y):
    """t at pixel (X, Y), Python ints"""
    T0, TX, TY = coeff
    return (T0 + X * TX + Y * TY) >> 16


def radial_t(x0, y0, R, X, Y):
    ddx, ddy = 64 * X + 32 - x0, 64 * Y + 32 - y0
    return (math.isqrt((ddx * ddx + ddy * ddy) * 256) * R) >> 48


def spread_u(t, spread):
    """t -> u in 0 .. 65535 (Python's % is the floor mod)"""
    if spread == PAD:
        return min(max(t, 0), 65535)
    if spread == REPEAT:
        return t % 65536
    v = t % 131072
    return v if v < 65536 else 131071 - v


def table(stops):
    """G[0 .. 1023] -> (1024, 4) int64"""
    off = [int(s[0]) for s in stops]
    col = [[int(v) for v in s[1]] for s in stops]
    n = len(stops)
    out = np.empty((1024, 4), np.int64)
    for k in range(1024):
        q = 64 * k + 32
        if q < off[0]:
            out[k] = col[0]
        elif q >= off[n - 1]:
            out[k] = col[n - 1]
        else:
            i = max(j for j in range(n) if off[j] <= q)
            wd, f = off[i + 1] - off[i], q - off[i]
            out[k] = [(col[i][c] * (wd - f) + col[i + 1][c] * f + wd // 2) // wd for c in range(4)]
    return out


def parameter(grad, X0, Y0, X1, Y1):
    """u of every pixel of [X0, X1) x [Y0, Y1) -> (Y1 - Y0, X1 - X0) int64"""
    kind, spread, (x0, y0, x1, y1), _ = grad
    u = np.empty((Y1 - Y0, X1 - X0), np.int64)
    if kind == LINEAR:
        c = linear_coefficients(x0, y0, x1, y1)
        for Y in range(Y0, Y1):
            for X in range(X0, X1):
                u[Y - Y0, X - X0] = spread_u(linear_t(c, X, Y), spread)
    else:
        R = radial_coefficient(x1)
        for Y in range(Y0, Y1):
            for X in range(X0, X1):
                u[Y - Y0, X - X0] = spread_u(radial_t(x0, y0, R, X, Y), spread)
    return u


def clip(window, dst, dst_stride, dst_rows):
    """(src_x, src_y, w, h), (dst_x, dst_y) -> (X0, Y0, X1, Y1, sx, sy) in the destination, or None"""
    return lr.clip((*window, *dst, 255), dst_stride, dst_rows)


def paint(image, layer, window, dst, grad, srgb=False):
    """fr_layer_paint on the host: image (dst_rows, dst_stride, 4) u8; layer (src_rows, src_stride, 4) u8 or None (full
    coverage); window (src_x, src_y, w, h); dst (dst_x, dst_y) -> a new image"""
    out = np.array(image, np.uint8, copy=True)
    c = clip(window, dst, out.shape[1], out.shape[0])
    if c is None:
        return out
    X0, Y0, X1, Y1, sx, sy = c
    colour = table(grad[3])[parameter(grad, X0, Y0, X1, Y1) >> 6]                  # (h, w, 4)
    cov = np.full((Y1 - Y0, X1 - X0), 255, np.int64) if layer is None else layer[sy:sy + Y1 - Y0, sx:sx + X1 - X0, 3].astype(np.int64)
    a = lr.m(cov, colour[..., 3])
    d = out[Y0:Y1, X0:X1].astype(np.int64)
    new = np.empty_like(d)
    for ch in range(3):
        if srgb:
            D, E = lr.srgb_tables()
            new[..., ch] = E[np.minimum(65535, (D[colour[..., ch]] * a + 127) // 255 + (D[d[..., ch]] * (255 - a) + 127) // 255)]
        else:
            new[..., ch] = np.minimum(255, lr.m(colour[..., ch], a) + lr.m(d[..., ch], 255 - a))
    new[..., 3] = a + lr.m(d[..., 3], 255 - a)
    out[Y0:Y1, X0:X1] = np.where((a > 0)[..., None], new, d).astype(np.uint8)       # a = 0: byte-identical
    return out

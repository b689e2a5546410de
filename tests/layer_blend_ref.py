"""numpy twin of fr_layer_blend (include/fr_raster.h): integer arithmetic only (int64; N stays below 3 * 65535^2 < 2^34),
written from the header's definition.  D and E come from where the other layer twins take them (tests/layer_ref.py); the
clipping is fr_layer_over's."""
import numpy as np

import layer_ref as R

MULTIPLY, SCREEN, OVERLAY, DARKEN, LIGHTEN, HARD_LIGHT, DIFFERENCE, EXCLUSION, PLUS = range(9)
MODES = 9
NAMES = ("multiply", "screen", "overlay", "darken", "lighten", "hard_light", "difference", "exclusion", "plus")
SYMMETRIC = (MULTIPLY, SCREEN, DARKEN, LIGHTEN, DIFFERENCE, EXCLUSION, PLUS)


def _pos(v):
    return np.maximum(v, 0)


def b2(mode, x, y, p, q):
    """the header's B2 = as ab B(Cb, Cs) on premultiplied terms: int64 arrays (or Python ints) in, the same out"""
    light = _pos(p * q - 2 * _pos(q - y) * _pos(p - x))
    if mode == MULTIPLY:
        return x * y
    if mode == SCREEN:
        return _pos(x * q + y * p - x * y)
    if mode == DARKEN:
        return np.minimum(x * q, y * p)
    if mode == LIGHTEN:
        return np.maximum(x * q, y * p)
    if mode == DIFFERENCE:
        return np.abs(x * q - y * p)
    if mode == EXCLUSION:
        return _pos(x * q + y * p - 2 * x * y)
    if mode == HARD_LIGHT:
        return np.where(2 * x <= p, 2 * x * y, light)
    if mode == OVERLAY:
        return np.where(2 * y <= q, 2 * x * y, light)
    raise ValueError(f"mode {mode}")


def numerator(mode, x, y, p, q, Q):
    """N of the header"""
    return x * (Q - q) + y * (Q - p) + b2(mode, x, y, p, q)


def channel(mode, x, y, p, q, Q):
    """`out` of the header for one colour byte, before E: x under p into y under q, all in [0, Q]"""
    x, y, p, q = (np.asarray(v, np.int64) for v in (x, y, p, q))
    if mode == PLUS:
        return np.minimum(Q, x + y)
    return np.minimum(Q, (numerator(mode, x, y, p, q, Q) + (Q - 1) // 2) // Q)


def blend(src, dst, o, mode, srgb=False):
    """src blended into dst: (..., 4) u8 arrays of premultiplied pixels, alpha last; o: the opacity, a scalar or an array
    that broadcasts against the pixels -> (..., 4) u8"""
    src, dst = np.asarray(src, np.uint8).astype(np.int64), np.asarray(dst, np.uint8).astype(np.int64)
    o = np.asarray(o, np.int64)
    out = np.empty(np.broadcast(src[..., 0], dst[..., 0], o).shape + (4,), np.uint8)
    a1, da = R.m(src[..., 3], o), dst[..., 3]
    for c in range(3):
        if not srgb:
            out[..., c] = channel(mode, R.m(src[..., c], o), dst[..., c], a1, da, 255)
        else:
            D, E = R.srgb_tables()
            out[..., c] = E[channel(mode, (D[src[..., c]] * o + 127) // 255, D[dst[..., c]], 257 * a1, 257 * da, 65535)]
    out[..., 3] = np.minimum(255, a1 + da) if mode == PLUS else a1 + R.m(da, 255 - a1)
    return out


def composite(layer, image, blits, mode, srgb=False):
    """fr_layer_blend on the host: layer (src_rows, src_stride, 4), image (dst_rows, dst_stride, 4) -> a new image"""
    out = np.array(image, np.uint8, copy=True)
    for b in blits:
        c = R.clip(b, image.shape[1], image.shape[0])
        if c is None:
            continue
        x0, y0, x1, y1, sx, sy = c
        out[y0:y1, x0:x1] = blend(layer[sy:sy + y1 - y0, sx:sx + x1 - x0], image[y0:y1, x0:x1], int(b[6]), mode, srgb)
    return out

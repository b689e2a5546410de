"""numpy twin of fr_layer_rects (include/fr_raster.h): integer arithmetic only, written from the header's definition,
rectangle by rectangle in the caller's order, each over the result of the ones before.  The sRGB tables come from
layer_ref.srgb_tables (the library's host functions)."""
import numpy as np

import layer_ref as lr


def overlap(lo, hi, n):
    """cx (or cy) for pixels 0 .. n - 1: the 1/64 pixels of [lo, hi) inside each, 0 .. 64 -> int64 array"""
    p = 64 * np.arange(n, dtype=np.int64)
    return np.maximum(0, np.minimum(int(hi), p + 64) - np.maximum(int(lo), p))


def coverage(rect, width, height):
    """k(X, Y) of a rectangle (x0, y0, x1, y1, ...) over a width x height image -> (height, width) int64"""
    x0, y0, x1, y1 = (int(v) for v in rect[:4])
    return (255 * overlap(y0, y1, height)[:, None] * overlap(x0, x1, width)[None, :] + 2048) // 4096


def bounding_box(rect, width, height):
    """the outward-rounded, clipped bounding box in pixels -> (X0, Y0, X1, Y1), or None when it is empty"""
    x0, y0, x1, y1 = (int(v) for v in rect[:4])
    X0, Y0, X1, Y1 = max(x0 // 64, 0), max(y0 // 64, 0), min(-(-x1 // 64), width), min(-(-y1 // 64), height)
    return (X0, Y0, X1, Y1) if X0 < X1 and Y0 < Y1 else None


def rects(image, rows, srgb=False):
    """fr_layer_rects on the host: image (dst_rows, dst_stride, 4) u8, rows of (x0, y0, x1, y1, (R, G, B, A)) with the edges
    in 1/64 pixel -> a new image"""
    out = np.array(image, np.uint8, copy=True)
    h, w = out.shape[:2]
    for row in rows:
        colour = [int(v) for v in row[4]]
        box = bounding_box(row, w, h)
        if box is None:
            continue
        X0, Y0, X1, Y1 = box
        a = lr.m(coverage(row, w, h)[Y0:Y1, X0:X1], colour[3])
        d = out[Y0:Y1, X0:X1].astype(np.int64)
        new = np.empty_like(d)
        for c in range(3):
            if srgb:
                D, E = lr.srgb_tables()
                new[..., c] = E[np.minimum(65535, (D[colour[c]] * a + 127) // 255 + (D[d[..., c]] * (255 - a) + 127) // 255)]
            else:
                new[..., c] = np.minimum(255, lr.m(colour[c], a) + lr.m(d[..., c], 255 - a))
        new[..., 3] = a + lr.m(d[..., 3], 255 - a)
        out[Y0:Y1, X0:X1] = np.where((a > 0)[..., None], new, d).astype(np.uint8)       # a = 0: byte-identical
    return out

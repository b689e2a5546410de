"""numpy twin of fr_layer_shadow (include/fr_raster.h): integer arithmetic only, written from the header's definition: pad
with zeros, take the maximum and the sums by shifted adds, round each pass once, then tint.  The sRGB tables come from
layer_ref.srgb_tables (the library's host functions)."""
import numpy as np

import layer_ref as lr


def reach(s, r, p):
    """R = s + p r (r = 0 or p = 0: no blur)"""
    return s + (p * r if r and p else 0)


def _shifted(a, k, op):
    """a (zero beyond its edges) combined over the (2 k + 1)^2 square, on a by k pixels larger on every side"""
    h, w = a.shape
    pad = np.zeros((h + 4 * k, w + 4 * k), np.int64)
    pad[2 * k:2 * k + h, 2 * k:2 * k + w] = a
    rows = None
    for i in range(2 * k + 1):
        part = pad[:, i:i + w + 2 * k]
        rows = part.copy() if rows is None else op(rows, part)
    out = None
    for j in range(2 * k + 1):
        part = rows[j:j + h + 2 * k, :]
        out = part.copy() if out is None else op(out, part)
    return out


def alpha_plane(a0, s, r, p):
    """A_last on the window grown by R on every side: a0 is (h, w) -> (h + 2 R, w + 2 R) int64; element (R + v, R + u) is
    A_last(u, v)"""
    a = np.asarray(a0).astype(np.int64)
    if s:
        a = _shifted(a, s, np.maximum)
    if r and p:
        W = (2 * r + 1) ** 2
        for _ in range(p):
            a = (_shifted(a, r, np.add) + W // 2) // W
    return a


def tint(alpha, rgba, srgb=False):
    """alpha (...) -> (..., 4) u8: the stored premultiplied element"""
    a = lr.m(alpha, int(rgba[3]))
    out = np.empty(a.shape + (4,), np.uint8)
    for c in range(3):
        if srgb:
            D, E = lr.srgb_tables()
            out[..., c] = E[(D[int(rgba[c])] * a + 127) // 255]
        else:
            out[..., c] = lr.m(int(rgba[c]), a)
    out[..., 3] = a
    return out


def shadow_rect(layer, window, size, offset, s, r, p, rgba, srgb=False):
    """the dst_h x dst_w x 4 pixels fr_layer_shadow writes: layer (rows, stride, 4) u8, window = (src_x, src_y, w, h),
    size = (dst_w, dst_h), offset = (dx, dy)"""
    sx, sy, w, h = window
    dw, dh = size
    dx, dy = offset
    R = reach(s, r, p)
    alpha = np.zeros((dh, dw), np.int64)
    if w and h and dw and dh:
        plane = alpha_plane(layer[sy:sy + h, sx:sx + w, 3], s, r, p)          # covers u in [-R, w + R), v in [-R, h + R)
        # destination (X, Y) shows (X - dx, Y - dy): plane index (Y - dy + R, X - dx + R)
        x0, x1 = max(0, dx - R), min(dw, dx + w + R)
        y0, y1 = max(0, dy - R), min(dh, dy + h + R)
        if x0 < x1 and y0 < y1:
            alpha[y0:y1, x0:x1] = plane[y0 - dy + R:y1 - dy + R, x0 - dx + R:x1 - dx + R]
    return tint(alpha, rgba, srgb)


def shadow(layer, image, window, rect, offset, s, r, p, rgba, srgb=False):
    """fr_layer_shadow on the host: image (dst_rows, dst_stride, 4) with rect = (dst_x, dst_y, dst_w, dst_h) -> a new image"""
    out = np.array(image, np.uint8, copy=True)
    x, y, dw, dh = rect
    if dw and dh:
        out[y:y + dh, x:x + dw] = shadow_rect(layer, window, (dw, dh), offset, s, r, p, rgba, srgb)
    return out

"""numpy twin of fr_layer_warp (include/fr_raster.h): int64 arithmetic only, written from the header's definition.  The
composite of the UNORM sample is layer_ref.over; the linear-light composite with S_c in the place of D[s_c] is written out.
The sRGB tables come from layer_ref.srgb_tables (the library's host functions)."""
import numpy as np

import layer_ref as lr
from font_renderer_amd import _lib

ONE, HALF = 65536, 32768
# a blit row is read in the order of fr_layer_warp_blit's fields, without the reserved word
FIELDS = tuple(name for name, _ in _lib.LayerWarpBlit._fields_)[:15]
assert FIELDS == ("src_x", "src_y", "w", "h", "dst_x", "dst_y", "dst_w", "dst_h", "u0", "v0", "ux", "uy", "vx", "vy", "opacity")


def identity(window, dst, opacity=255, a=0, b=0):
    """consequence 1's blit: the rectangle of the window's size at dst, showing the window moved by (a, b) whole pixels"""
    sx, sy, w, h = window
    return (sx, sy, w, h, dst[0], dst[1], w, h, HALF + ONE * a, HALF + ONE * b, ONE, 0, 0, ONE, opacity)


def symmetries(w, h):
    """(numpy turn of the (h, w) layer, the blit's map for a rectangle at its size) for the eight quarter turns and mirrors"""
    E = (w - 1) * ONE + HALF, (h - 1) * ONE + HALF             # the centres of the last column and row
    return {
        "identity": (lambda a: a, (HALF, HALF, ONE, 0, 0, ONE)),
        "mirror_x": (lambda a: a[:, ::-1], (E[0], HALF, -ONE, 0, 0, ONE)),
        "mirror_y": (lambda a: a[::-1], (HALF, E[1], ONE, 0, 0, -ONE)),
        "half_turn": (lambda a: a[::-1, ::-1], (E[0], E[1], -ONE, 0, 0, -ONE)),
        "transpose": (lambda a: a.swapaxes(0, 1), (HALF, HALF, 0, ONE, ONE, 0)),
        "quarter_turn": (lambda a: a.swapaxes(0, 1)[:, ::-1], (HALF, E[1], 0, ONE, -ONE, 0)),        # out[y, x] = a[h - 1 - x, y]
        "three_quarter_turn": (lambda a: a.swapaxes(0, 1)[::-1], (E[0], HALF, 0, -ONE, ONE, 0)),     # out[y, x] = a[x, w - 1 - y]
        "anti_transpose": (lambda a: a.swapaxes(0, 1)[::-1, ::-1], (E[0], E[1], 0, -ONE, -ONE, 0)),
    }


def coordinates(blit, X, Y):
    """U and V of rectangle pixels (X, Y), int64 arrays that broadcast"""
    u0, v0, ux, uy, vx, vy = (int(v) for v in blit[8:14])
    X, Y = np.asarray(X, np.int64), np.asarray(Y, np.int64)
    return u0 + X * ux + Y * uy, v0 + X * vx + Y * vy


def taps(window_px, U, V):
    """the four taps p(i, j), p(i+1, j), p(i, j+1), p(i+1, j+1) as (..., 4) int64 arrays, (0, 0, 0, 0) outside the window,
    with fx, fy and whether any of the four is inside the window"""
    h, w = window_px.shape[:2]
    P, Q = U - HALF, V - HALF
    i, j = P >> 16, Q >> 16
    fx, fy = (P & 0xffff) >> 8, (Q & 0xffff) >> 8
    out, hit = [], np.zeros(np.broadcast(i, j).shape, bool)
    for dj in (0, 1):
        for di in (0, 1):
            ii, jj = np.broadcast_arrays(i + di, j + dj)
            inside = (ii >= 0) & (ii < w) & (jj >= 0) & (jj < h)
            px = window_px[np.clip(jj, 0, h - 1), np.clip(ii, 0, w - 1)].astype(np.int64)
            out.append(np.where(inside[..., None], px, 0))
            hit |= inside
    return out, fx, fy, hit


def bilerp(p00, p10, p01, p11, fx, fy):
    """the header's formula on int64 arrays of bytes or of 16-bit linear values"""
    top = p00 * (256 - fx) + p10 * fx
    bot = p01 * (256 - fx) + p11 * fx
    return (top * (256 - fy) + bot * fy + 32768) >> 16


def sample(window_px, U, V, srgb=False):
    """(s, S): s the (..., 4) sampled bytes (with srgb only its alpha is the definition's), S the (..., 3) linear colour
    samples or None; and the hit mask"""
    (p00, p10, p01, p11), fx, fy, hit = taps(window_px, U, V)
    f = fx[..., None], fy[..., None]
    s = bilerp(p00, p10, p01, p11, *f)
    if not srgb:
        return s, None, hit
    D, _ = lr.srgb_tables()
    S = bilerp(D[p00[..., :3]], D[p10[..., :3]], D[p01[..., :3]], D[p11[..., :3]], *f)
    return s, S, hit


def over_sample(s, S, dst, o, srgb=False):
    """the sample composited over dst (..., 4) u8 at opacity o -> (..., 4) u8"""
    if not srgb:
        return lr.over(s.astype(np.uint8), dst, o, False)
    D, E = lr.srgb_tables()
    d = np.asarray(dst, np.uint8).astype(np.int64)
    a1 = lr.m(s[..., 3], o)
    out = np.empty(d.shape, np.uint8)
    for c in range(3):
        out[..., c] = E[np.minimum(65535, (S[..., c] * o + 127) // 255 + (D[d[..., c]] * (255 - a1) + 127) // 255)]
    out[..., 3] = a1 + lr.m(d[..., 3], 255 - a1)
    return out


def clip(blit, dst_stride, dst_rows):
    """the rectangle of a blit clipped to the image -> (x0, y0, x1, y1) or None"""
    dx, dy, dw, dh = (int(v) for v in blit[4:8])
    x0, y0, x1, y1 = max(dx, 0), max(dy, 0), min(dx + dw, dst_stride), min(dy + dh, dst_rows)
    return None if dw == 0 or dh == 0 or x0 >= x1 or y0 >= y1 else (x0, y0, x1, y1)


def composite(layer, image, blits, srgb=False, hits=None):
    """fr_layer_warp on the host: layer (src_rows, src_stride, 4), image (dst_rows, dst_stride, 4), blits rows of FIELDS
    -> a new image.  hits: a bool array of the image's shape that is set where a pixel has a tap in its window."""
    out = np.array(image, np.uint8, copy=True)
    for b in blits:
        sx, sy, w, h = (int(v) for v in b[:4])
        c = clip(b, image.shape[1], image.shape[0])
        if c is None or w == 0 or h == 0:
            continue
        x0, y0, x1, y1 = c
        U, V = coordinates(b, np.arange(x0, x1)[None, :] - int(b[4]), np.arange(y0, y1)[:, None] - int(b[5]))
        s, S, hit = sample(layer[sy:sy + h, sx:sx + w], U, V, srgb)
        if hits is not None:
            hits[y0:y1, x0:x1] |= hit
        out[y0:y1, x0:x1] = over_sample(s, S, image[y0:y1, x0:x1], int(b[14]), srgb)
    return out

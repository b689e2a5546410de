"""numpy / Python-int twin of fr_layer_lcd (include/fr_raster.h): integer arithmetic only, written from the header's
definition.  A blit is (src_x, src_y, w, h, dst_x, dst_y, (R, G, B, A)); the flags are the header's (SRGB = 1, BGR = 2).
m and the sRGB tables are layer_ref's (the library's host functions)."""
import numpy as np

import layer_ref as lr

SRGB, BGR, TAPS = 1, 2, 5
DEFAULT = (8, 77, 86, 77, 8)
IDENTITY = (0, 0, 256, 0, 0)


def window(plane, blit):
    """c(q, v) of the blit for 0 <= q < 3 w, with two zero elements on either side -> (h, 3 w + 4) int64"""
    sx, sy, w, h = (int(v) for v in blit[:4])
    c = np.zeros((h, 3 * w + 4), np.int64)
    c[:, 2:2 + 3 * w] = plane[sy:sy + h, sx:sx + 3 * w]
    return c


def filtered(plane, blit, weights=None):
    """f of every sub-pixel of the window -> (h, w, 3) int64, [..., j] sub-pixel j"""
    W = DEFAULT if weights is None else tuple(int(v) for v in weights)
    assert len(W) == TAPS and sum(W) == 256
    c = window(plane, blit)
    n = c.shape[1] - 4
    s = sum(W[i] * c[:, i:i + n] for i in range(TAPS))          # element q + i - 2 of the window is column q + i here
    return ((s + 128) // 256).reshape(c.shape[0], n // 3, 3)


def composite_px(colour, f, d, srgb):
    """the header's composite: colour (R, G, B, A); f (..., 3) what each memory byte takes; d (..., 4) -> (..., 4) int64"""
    a = lr.m(f, colour[3])
    out = np.empty_like(d)
    for b in range(3):
        if srgb:
            D, E = lr.srgb_tables()
            out[..., b] = E[np.minimum(65535, (D[colour[b]] * a[..., b] + 127) // 255 + (D[d[..., b]] * (255 - a[..., b]) + 127) // 255)]
        else:
            out[..., b] = np.minimum(255, lr.m(colour[b], a[..., b]) + lr.m(d[..., b], 255 - a[..., b]))
    amax = a.max(-1)
    out[..., 3] = amax + lr.m(d[..., 3], 255 - amax)
    return out


def lcd(plane, image, blits, weights=None, flags=0):
    """fr_layer_lcd on the host: plane (cov_rows, cov_stride) u8, image (dst_rows, dst_stride, 4) u8 -> a new image"""
    plane = np.asarray(plane, np.uint8)
    out = np.array(image, np.uint8, copy=True)
    for bl in blits:
        c = lr.clip((*bl[:6], 255), image.shape[1], image.shape[0])
        if c is None:
            continue
        x0, y0, x1, y1, _, _ = c
        u0, v0 = x0 - int(bl[4]), y0 - int(bl[5])
        f = filtered(plane, bl, weights)[v0:v0 + y1 - y0, u0:u0 + x1 - x0]
        if flags & BGR:
            f = f[..., ::-1]
        out[y0:y1, x0:x1] = composite_px([int(v) for v in bl[6]], f, image[y0:y1, x0:x1].astype(np.int64), bool(flags & SRGB)).astype(np.uint8)
    return out

"""numpy twin of fr_layer_mask (include/fr_raster.h): integer arithmetic only, written from the header's definition.  The
composite is layer_ref.over with the per-pixel t = m(k', o) as its opacity; the erase is written out.  The sRGB tables come
from layer_ref.srgb_tables (the library's host functions)."""
import numpy as np

import layer_ref as lr


def t_of(k, o, invert=False):
    """t = m(k', o), k' = 255 - k when inverting; k an array or a scalar"""
    k = np.asarray(k, np.int64)
    return lr.m(255 - k if invert else k, o)


def erase(dst, t, srgb=False):
    """dst (..., 4) u8 premultiplied pixels, alpha last, times 255 - t; t: a scalar or an array that broadcasts
    against the pixels, as layer_ref.over's o -> (..., 4) u8"""
    d = np.asarray(dst, np.uint8).astype(np.int64)
    ia = 255 - np.asarray(t, np.int64)
    out = np.empty(d.shape, np.uint8)
    for c in range(3):
        if srgb:
            D, E = lr.srgb_tables()
            out[..., c] = E[(D[d[..., c]] * ia + 127) // 255]
        else:
            out[..., c] = lr.m(d[..., c], ia)
    out[..., 3] = lr.m(d[..., 3], ia)
    return out


def mask_values(mask):
    """k of every element: the alpha of a (rows, stride, 4) layer mask, or a (rows, stride) plane as it is"""
    mask = np.asarray(mask, np.uint8)
    return mask[..., 3] if mask.ndim == 3 else mask


def composite(layer, mask, image, blits, srgb=False, erase_mode=False):
    """fr_layer_mask on the host: layer (src_rows, src_stride, 4) or None when erasing; mask (rows, stride, 4), a layer, or
    (rows, stride), a plane; image (dst_rows, dst_stride, 4); blits rows of (src_x, src_y, w, h, dst_x, dst_y, mask_x,
    mask_y, opacity, invert) -> a new image, with layer_ref.clip's geometry"""
    out = np.array(image, np.uint8, copy=True)
    k = mask_values(mask)
    for b in blits:
        sx, sy, w, h, dx, dy, mx, my, o, inv = (int(v) for v in b)
        if erase_mode:
            sx = sy = 0
        c = lr.clip((sx, sy, w, h, dx, dy, o), image.shape[1], image.shape[0])
        if c is None:
            continue
        x0, y0, x1, y1, cx, cy = c
        mx, my = mx + (cx - sx), my + (cy - sy)
        t = t_of(k[my:my + y1 - y0, mx:mx + x1 - x0], o, inv)
        assert t.shape == (y1 - y0, x1 - x0), "the rectangle leaves the mask"
        if erase_mode:
            out[y0:y1, x0:x1] = erase(image[y0:y1, x0:x1], t, srgb)
        else:
            out[y0:y1, x0:x1] = lr.over(layer[cy:cy + y1 - y0, cx:cx + x1 - x0], image[y0:y1, x0:x1], t, srgb)
    return out

"""numpy twin of fr_layer_over and fr_layer_unpremultiply (include/fr_raster.h): integer arithmetic only, written from
the header's definition.  The sRGB tables D and E come from the library's host functions fr_srgb_decode / fr_srgb_encode
(no GPU), which tests/test_text_srgb_ref.py holds to the IEC formula."""
import numpy as np

import font_renderer_amd as fr

_tables = {}


def srgb_tables():
    """(D[256] as int64, E[65536] as int64)"""
    if not _tables:
        _tables["D"] = fr.srgb_to_linear16(np.arange(256, dtype=np.uint8)).astype(np.int64)
        _tables["E"] = fr.linear16_to_srgb(np.arange(65536, dtype=np.uint16)).astype(np.int64)
    return _tables["D"], _tables["E"]


def m(x, y):
    """(x * y + 127) div 255"""
    return (np.asarray(x, np.int64) * np.asarray(y, np.int64) + 127) // 255


def over_alpha(s_a, d_a, o):
    a1 = m(s_a, o)
    return a1 + m(d_a, 255 - a1)


def over_colour_raw(s_c, s_a, d_c, o, srgb=False):
    """one colour channel before the clamp (UNORM) / the linear sum before the clamp and E (sRGB)"""
    ia = 255 - m(s_a, o)
    if not srgb:
        return m(s_c, o) + m(d_c, ia)
    D, _ = srgb_tables()
    return (D[s_c] * np.asarray(o, np.int64) + 127) // 255 + (D[d_c] * ia + 127) // 255


def over_colour(s_c, s_a, d_c, o, srgb=False):
    raw = over_colour_raw(s_c, s_a, d_c, o, srgb)
    if not srgb:
        return np.minimum(255, raw)
    return srgb_tables()[1][np.minimum(65535, raw)]


def over(src, dst, o, srgb=False):
    """src over dst: (..., 4) u8 arrays of premultiplied pixels, alpha last; o: the opacity, a scalar or an array that
    broadcasts against the pixels -> (..., 4) u8"""
    src, dst = np.asarray(src, np.uint8).astype(np.int64), np.asarray(dst, np.uint8).astype(np.int64)
    o = np.asarray(o, np.int64)
    out = np.empty(np.broadcast(src, dst).shape, np.uint8)
    for c in range(3):
        out[..., c] = over_colour(src[..., c], src[..., 3], dst[..., c], o, srgb)
    out[..., 3] = over_alpha(src[..., 3], dst[..., 3], o)
    return out


def clip(blit, dst_stride, dst_rows):
    """an (src_x, src_y, w, h, dst_x, dst_y, opacity) row -> (x0, y0, x1, y1, sx, sy) in the destination, or None"""
    sx, sy, w, h, dx, dy, _ = (int(v) for v in blit)
    x0, y0, x1, y1 = max(dx, 0), max(dy, 0), min(dx + w, dst_stride), min(dy + h, dst_rows)
    if w == 0 or h == 0 or x0 >= x1 or y0 >= y1:
        return None
    return x0, y0, x1, y1, sx + x0 - dx, sy + y0 - dy


def composite(layer, image, blits, srgb=False):
    """fr_layer_over on the host: layer (src_rows, src_stride, 4), image (dst_rows, dst_stride, 4) -> a new image"""
    out = np.array(image, np.uint8, copy=True)
    for b in blits:
        c = clip(b, image.shape[1], image.shape[0])
        if c is None:
            continue
        x0, y0, x1, y1, sx, sy = c
        out[y0:y1, x0:x1] = over(layer[sy:sy + y1 - y0, sx:sx + x1 - x0], image[y0:y1, x0:x1], int(b[6]), srgb)
    return out


def unpremultiply(px, srgb=False):
    """fr_rgba_unpremultiply's three cases on (..., 4) u8 pixels -> a new array"""
    px = np.asarray(px, np.uint8)
    v = px.astype(np.int64)
    a = v[..., 3]
    safe = np.maximum(a, 1)
    out = px.copy()
    for c in range(3):
        if srgb:
            D, E = srgb_tables()
            q = E[np.minimum(65535, (255 * D[v[..., c]] + safe // 2) // safe)]
        else:
            q = np.minimum(255, (255 * v[..., c] + safe // 2) // safe)
        out[..., c] = np.where(a == 0, 0, q)
    return out

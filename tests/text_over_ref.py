"""The expected image of an FR_TEXT_OVER text plan (include/fr_raster.h), assembled from the twins of the plan without the
flag: this module holds no rasterisation and no blend of its own.
  R, G, B: the twin of the same plan without the flag (tests/text_rgba_ref.py, text_srgb_ref.py, text_load_ref.py for
      fr_glyph_place; text_place_ref.py for fr_glyph_place_ex; text_affine_ref.py for fr_glyph_place_affine).
  Alpha: the R channel of the UNORM twin of the same placements with every placement colour (255, 255, 255, A_k), every
      clear colour (a, a, a, a) from its alpha and, under FR_TEXT_LOAD, every stored pixel (a, a, a, a): the alpha update
      a' = (255 A + a (255 - A) + 127) div 255 is the colour update with C = 255, and alpha resolves as a UNORM channel in
      both colour spaces."""
import numpy as np

import text_affine_ref as ta
import text_load_ref as tl
import text_place_ref as tp
import text_rgba_ref as tr
import text_srgb_ref as ts

FORMS = ("plain", "ex", "affine")


def alpha_over(a, A):
    """the definition's alpha update, in integers (arrays or ints)"""
    return (255 * A + a * (255 - A) + 127) // 255


def plain_twin(form, gs, places, cols, runs, clears, out, n, center, fill, srgb, bgr, load):
    """the twin of the plan WITHOUT the flag, drawn into `out` in place -> out.  form: which placement record `places` holds"""
    if form == "ex":
        return tp.rgba_render_runs(gs, places, cols, runs, clears, out, n, center, fill, srgb, bgr, load)
    if form == "affine":
        return ta.rgba_render_runs(gs, places, cols, runs, clears, out, n, center, fill, srgb, bgr, load)
    assert form == "plain", form
    if load:
        return tl.render_runs(gs, places, cols, runs, out, n, center, fill, srgb, bgr)
    if srgb:
        return ts.render_runs(gs, places, cols, runs, clears, out, n, center, fill, bgr=bgr)
    if bgr:         # FR_TEXT_BGRA is R and B swapped in every placement and clear colour (include/fr_raster.h)
        return tr.render_runs(gs, places, ts.bgra(np.asarray(cols)), runs, ts.bgra(np.asarray(clears)), out, n, center, fill)
    return tr.render_runs(gs, places, cols, runs, clears, out, n, center, fill)


def render_runs(form, gs, places, cols, runs, clears, start, n=1, center=False, fill=False, srgb=False, bgr=False, load=False):
    """start: the (rows, cols, 4) u8 buffer before the render (the sentinel, or under FR_TEXT_LOAD the stored pixels, in
    the stored byte order) -> the buffer after the render of the plan with FR_TEXT_OVER; start is left as it is"""
    start = np.asarray(start, np.uint8)
    cols = np.asarray(cols, np.uint8)
    out = plain_twin(form, gs, places, cols, runs, clears, start.copy(), n, center, fill, srgb, bgr, load)
    white = cols.copy()
    white[:, :3] = 255
    gray_clears = None if clears is None else np.repeat(np.asarray(clears, np.uint8)[:, 3:], 4, axis=1)
    gray_start = np.repeat(start[..., 3:], 4, axis=-1)
    alpha = plain_twin(form, gs, places, white, runs, gray_clears, gray_start, n, center, fill, False, False, load)
    out[..., 3] = alpha[..., 0]
    return out

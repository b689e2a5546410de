"""Text runs: a string laid out by the reference's pen walk (Appli.zig:318-349) and rendered as one anti-aliased image
through a text plan (fr_text_plan_create, include/fr_raster.h), or as one RGBA image through an RGBA text plan
(fr_text_plan_create_rgba), or drawn over an RGBA image the caller has (FR_TEXT_LOAD).  A slant, a fractional baseline,
spans of several sizes on one baseline (render_spans) and the reference's zoomed and dragged frame (render_text_view)
go through the placement form of those plans (fr_glyph_place_ex); a line along any direction (render_text_rotated) goes
through the matrix form (fr_glyph_place_affine).  Nothing is computed in Python but the image size
and the pen positions."""
from __future__ import annotations

import math
from contextlib import closing
from typing import Optional

import numpy as np

from . import _lib as L
from .device import Context, default_context, round_trip
from .font import Font
from .image import RGBA, Gray, colour_rgba, q64, rgba_pixels
from .layer import layer_lcd, make_lcd_blits
from .render_glyph import DeviceGlyphSet, TextPlan, TextPlanRGBA, make_places, make_places_affine, make_places_ex, make_runs


def instance_cell(box, scale: float, pen_x64: int, pen_y: int):
    """an instance's cell in image coordinates, unclipped -> (column 0, row 0, width, height): renderGlyph's grid at
    `scale` (binary32 as render_glyph.zig:13-17), one column wider when the pen has a fractional part"""
    s = np.float32(scale)
    b = np.asarray(box, np.int16).astype(np.float32) * s
    mn_x, mn_y = math.floor(b[0]), math.floor(b[1])
    mx_x, mx_y = math.ceil(b[2]), math.ceil(b[3])
    ix, fx64 = pen_x64 >> 6, pen_x64 & 63
    return ix + mn_x, pen_y - mx_y, mx_x - mn_x + 1 + (fx64 != 0), mx_y - mn_y + 1


def instance_cell_ex(box, scale: float, slant: float, pen_x64: int, pen_y64: int):
    """instance_cell for an fr_glyph_place_ex (include/fr_raster.h): the grid of the box sheared by `slant`, one column /
    row wider when the pen's x / y has a fractional part (binary32, one rounding per operation).  At slant 0 and a
    whole pen_y64 = 64 * pen_y it is instance_cell's (x + 0 * y == x in binary32)."""
    f = np.float32
    s, k = f(scale), f(slant)
    x_min, y_min, x_max, y_max = (f(int(v)) for v in box)
    lo = min(f(x_min + f(k * y_min)), f(x_min + f(k * y_max)))
    hi = max(f(x_max + f(k * y_min)), f(x_max + f(k * y_max)))
    mn_x, mx_x = math.floor(f(lo * s)), math.ceil(f(hi * s))
    mn_y, mx_y = math.floor(f(y_min * s)), math.ceil(f(y_max * s))
    return ((pen_x64 >> 6) + mn_x, (pen_y64 >> 6) - mx_y, mx_x - mn_x + 1 + ((pen_x64 & 63) != 0),
            mx_y - mn_y + 1 + ((pen_y64 & 63) != 0))


def instance_cell_affine(box, m, pen_x64: int, pen_y64: int):
    """instance_cell for an fr_glyph_place_affine (include/fr_raster.h): the grid of the box's four corners mapped by
    m = (xx, xy, yx, yy), one column / row wider when the pen's x / y has a fractional part (binary32, one rounding per
    operation)"""
    f = np.float32
    xx, xy, yx, yy = (f(v) for v in m)
    x_min, y_min, x_max, y_max = (f(int(v)) for v in box)
    u = [f(f(xx * x) + f(xy * y)) for x in (x_min, x_max) for y in (y_min, y_max)]
    v = [f(f(yx * x) + f(yy * y)) for x in (x_min, x_max) for y in (y_min, y_max)]
    mn_x, mx_x, mn_y, mx_y = math.floor(min(u)), math.ceil(max(u)), math.floor(min(v)), math.ceil(max(v))
    return ((pen_x64 >> 6) + mn_x, (pen_y64 >> 6) - mx_y, mx_x - mn_x + 1 + ((pen_x64 & 63) != 0),
            mx_y - mn_y + 1 + ((pen_y64 & 63) != 0))


# ---- the small rules, each written once

def _slant(slant) -> float:
    k = float(slant)
    if not math.isfinite(k) or abs(k) > 4.0:
        raise ValueError(f"slant {slant!r}: expected a finite value in [-4, 4]")
    return k


def _zoom(zoom) -> float:
    zoom = float(zoom)
    if not (math.isfinite(zoom) and zoom > 0.0):
        raise ValueError(f"zoom {zoom!r}: expected a finite value > 0")
    return zoom


def _frame(width, height) -> None:
    """the size of an image that clips a line"""
    if not (isinstance(width, (int, np.integer)) and isinstance(height, (int, np.integer)) and 0 <= width <= 65535
            and 0 <= height <= 65535):
        raise ValueError(f"width {width!r} and height {height!r} must be integers in [0, 65535]")


def _flags(flags: int, srgb: bool = False, bgra: bool = False, cache: bool = False, over: bool = False, affine: bool = False) -> int:
    """the flag word of a text plan from the keyword arguments of the render functions; affine: the plan is of the matrix
    form, whose cache flag is FR_TEXT_CACHE_AFFINE"""
    return (flags | (L.FR_TEXT_SRGB if srgb else 0) | (L.FR_TEXT_BGRA if bgra else 0)
            | ((L.FR_TEXT_CACHE_AFFINE if affine else L.FR_TEXT_CACHE) if cache else 0) | (L.FR_TEXT_OVER if over else 0))


def _per_char(text, color, colors) -> list:
    """the colour of every character: colors[k], or `color` for all of them"""
    if colors is None:
        return [colour_rgba(color)] * len(text)
    if len(colors) != len(text):
        raise ValueError(f"colors: {len(colors)} colours for {len(text)} characters")
    return [colour_rgba(c) for c in colors]


def _scale(font: Font, font_size, zoom: float = 1.0) -> np.float32:
    """f32(f32(font_size) * f32(zoom)) / f32(units_per_em)"""
    return np.float32(font_size) * np.float32(zoom) / np.float32(font.information.units_per_em)


# ---- layout

def _glyphs(font: Font, glyph_indices):
    """the glyph set of the distinct glyphs of a line -> (glyph set, every entry's index in the set)"""
    gs, kept = font.glyphset(sorted({int(g) for g in glyph_indices}), skip_unsupported=False)
    local = {g: k for k, g in enumerate(kept)}
    return gs, [local[int(g)] for g in glyph_indices]


def _layout(font: Font, text, font_size: int, clipped_away: bool = False):
    """font.layout and the line's glyph set -> (glyph set, glyph k's index in the set, glyph k's pen_x64, end pen), or None
    for an empty text, and after the layout's own checks for an image that has no pixels (clipped_away)"""
    gi, pen, end = font.layout(text, font_size)
    if clipped_away or len(gi) == 0:
        return None
    return _glyphs(font, gi) + ([int(p) for p in pen], end)


def _fit(gs, rows, upright: bool = False):
    """rows of (local glyph, pen_x64, pen_y64, scale, slant) around the pen origin (0, 0) -> one run whose image is the
    union of the instance cells: (places, runs, width, height), or None when nothing is drawn.  The pen origin is at the
    image's left edge, moved right by whole pixels if a cell reaches left of it (the fractional pens stay as laid out),
    and the baseline at row -top = ceil(max y_max * scale).  upright: the rows have slant 0 and whole pen_y64, and the
    places are fr_glyph_place rows, which select the text_* kernels, instead of fr_glyph_place_ex rows."""
    seg = gs.segments_per_glyph()
    cells = [instance_cell_ex(gs.boxes[g], s, k, x, y) for g, x, y, s, k in rows if seg[g] > 0]
    if not cells:
        return None
    left = min(c[0] for c in cells)
    shift = -left if left < 0 else 0
    top = min(c[1] for c in cells)
    width = max(c[0] + c[2] for c in cells) + shift
    height = max(c[1] + c[3] for c in cells) - top
    if upright:
        places = make_places([(g, x + 64 * shift, (y >> 6) - top) for g, x, y, _, _ in rows])
    else:
        places = make_places_ex([(g, x + 64 * shift, y - 64 * top, s, k) for g, x, y, s, k in rows])
    runs = make_runs([(0, len(places), width, height, 0, 0, rows[0][3])])
    return places, runs, width, height


def _line(font: Font, text, font_size: int, slant: float = 0.0):
    """one line laid out as one run: (glyph set, places, runs, width, height), or None when nothing is drawn; sized by
    _fit.  An oblique line is in the placement form, cells of the sheared boxes."""
    laid = _layout(font, text, font_size)
    if laid is None:
        return None
    gs, local, pens, _ = laid
    scale = _scale(font, font_size)
    fit = _fit(gs, [(g, p, 0, scale, slant) for g, p in zip(local, pens)], upright=slant == 0.0)
    return None if fit is None else (gs,) + fit


# ---- rendering

def _render(ctx: Optional[Context], line, width: int, height: int, samples_per_axis: int, phase: int, flags: int,
            mode: int = L.FR_COVERAGE_U8, colours=None, clear=None, image: Optional[RGBA] = None):
    """line = (glyph set, places, runs) of any placement form through one plan, rendered once into width x height pixels
    -> Gray from a TextPlan in `mode`, or with per-placement `colours` RGBA from a TextPlanRGBA: over the colour `clear`, or
    with `image` over that image's pixels (FR_TEXT_LOAD in flags), which are replaced"""
    ctx = ctx or default_context()
    gs, places, runs = line
    if image is not None:
        target = image.data                                 # uploaded and drawn over
    else:
        target = (height * width,) if colours is None else (height * width, 4)    # a shape: allocated on the device
    with closing(DeviceGlyphSet(ctx, gs)) as dgs:
        if colours is None:
            plan = TextPlan(dgs, places, runs, mode, samples_per_axis, phase, flags)
        else:
            plan = TextPlanRGBA(dgs, places, colours, runs, None if clear is None else [clear], samples_per_axis, phase, flags)
        with closing(plan):
            out = round_trip(ctx, lambda p: plan.render(p, width, height), target)
    if image is not None:
        image.data[:] = out
        return image
    return Gray(width, height, out) if colours is None else RGBA(width, height, out)


def render_text(font: Font, text, font_size: int, *, samples_per_axis: int = 4, mode: int = L.FR_COVERAGE_U8,
                phase: int = L.FR_SAMPLE_CENTER, flags: int = 0, slant: float = 0.0, cache: bool = False,
                ctx: Optional[Context] = None) -> Gray:
    """One line of text as one image: every glyph at its sub-pixel pen, overlapping glyphs unioned per sample.
    The image is the union of the instance cells: the pen origin at its left edge (moved right by whole pixels if a cell
    reaches left of it) and the baseline at row ceil(max y_max * scale).  slant: a point (x, y) of every outline is drawn
    at (x + slant * y, y) (0.2: an oblique of about 11 degrees); the advances do not change.  cache: FR_TEXT_CACHE, the
    same bytes with each distinct (glyph, pen fraction) rasterised once; it pays when characters repeat at equal
    fractions and costs the mask store otherwise."""
    line = _line(font, text, font_size, _slant(slant))
    if line is None:
        return Gray.init(0, 0)
    return _render(ctx, line[:3], *line[3:], samples_per_axis, phase, _flags(flags, cache=cache), mode)


def render_text_rgba(font: Font, text, font_size: int, color=(225, 105, 180, 255), background=(0, 0, 0, 0), colors=None,
                     *, samples_per_axis: int = 4, phase: int = L.FR_SAMPLE_CENTER, flags: int = 0, srgb: bool = False,
                     bgra: bool = False, slant: float = 0.0, cache: bool = False, over: bool = False,
                     ctx: Optional[Context] = None) -> RGBA:
    """One line of text as one RGBA image (fr_text_plan_create_rgba): every glyph blended per sample in order over
    `background`, in `color` or, if `colors` is given, in colors[k] for character k (e.g. to highlight a word).  The
    defaults are the reference's frame: pink text (shader.slang) on a transparent clear colour.  Sized as render_text.
    srgb: blend and resolve in linear light, as the reference's sRGB swapchain does (FR_TEXT_SRGB); bgra: the pixels'
    bytes are B G R A (FR_TEXT_BGRA; the colours stay R G B A); slant and cache as render_text.  over: source-over
    alpha (FR_TEXT_OVER): a covered sample's alpha becomes A + a (1 - A) instead of A, so the image is then premultiplied
    (in linear light with srgb) and, over a transparent background, a layer that composites correctly over anything;
    RGBA.unpremultiply turns it into straight alpha.  R, G and B are those of over=False."""
    slant = _slant(slant)
    ctx = ctx or default_context()
    per_char, clear = _per_char(text, color, colors), colour_rgba(background)
    line = _line(font, text, font_size, slant)
    if line is None:
        return RGBA.init(0, 0)
    return _render(ctx, line[:3], *line[3:], samples_per_axis, phase, _flags(flags, srgb, bgra, cache, over), colours=per_char,
                   clear=clear)


def placed_line(font: Font, text, font_size: int, x: float, y: float, width: int, height: int, slant: float = 0.0):
    """The line draw_text_rgba draws: laid out at `font_size` with the pen origin at image x and the baseline at image y,
    both kept to 1/64 pixel (floor(64 v + 1/2)).  -> (glyph set, places, runs): one run of width x height pixels that
    clips the line, or None for an empty text or image.  The places are fr_glyph_place rows for an upright line on a
    whole pixel row (slant == 0 and pen_y64 a multiple of 64) and fr_glyph_place_ex rows otherwise."""
    slant = _slant(slant)
    if not math.isfinite(float(y)):
        raise ValueError(f"y {y!r}: expected a finite value")
    laid = _layout(font, text, font_size, width == 0 or height == 0)
    if laid is None:
        return None
    gs, local, pens, _ = laid
    x64, y64 = q64(x), q64(y)
    if slant == 0.0 and y64 % 64 == 0:
        places = make_places([(g, x64 + p, y64 // 64) for g, p in zip(local, pens)])
    else:
        places = make_places_ex([(g, x64 + p, y64, 0.0, slant) for g, p in zip(local, pens)])
    return gs, places, make_runs([(0, len(places), int(width), int(height), 0, 0, _scale(font, font_size))])


def draw_text_rgba(image: RGBA, font: Font, text, font_size: int, x: float, y: float, color=(225, 105, 180, 255), colors=None,
                   *, samples_per_axis: int = 4, phase: int = L.FR_SAMPLE_CENTER, flags: int = 0, srgb: bool = False,
                   bgra: bool = False, slant: float = 0.0, cache: bool = False, over: bool = False,
                   ctx: Optional[Context] = None) -> RGBA:
    """One line of text drawn in place into `image` (FR_TEXT_LOAD): every sample starts at the pixel already there, and
    the glyphs are blended over it per sample in order, in `color` or colors[k] for character k.  x: the pen origin's
    image x in pixels (fractional x is kept to 1/64 pixel: pen_x64 = floor(64 x + 1/2)); y: the baseline's image y, kept
    to 1/64 pixel likewise (pen_y64 = floor(64 y + 1/2); an integral y is that row); slant as render_text.  The
    line is one run covering the whole image (placed_line), so glyphs are clipped at its edges.  The whole image is copied to the
    device and back; on the device only the 64 x 16 tiles that some glyph cell meets are read (and, where needed,
    written), and every pixel no glyph sample reaches comes back with its bytes unchanged.  srgb / bgra as
    render_text_rgba: the image's bytes are sRGB / B G R A; cache as render_text.  image.data must be a (height * width, 4) uint8 array
    (ValueError otherwise).  over: source-over alpha (FR_TEXT_OVER): the image is then read and written as premultiplied
    R G B A, and translucent text leaves the alpha of an opaque picture at 255 (with over=False every covered sample's
    alpha becomes the colour's A).  Returns `image`."""
    w, h = image.width, image.height
    if not (isinstance(w, (int, np.integer)) and isinstance(h, (int, np.integer)) and w >= 0 and h >= 0):
        raise ValueError(f"image: width {w!r} and height {h!r} must be non-negative integers")
    rgba_pixels(image, "draw_text_rgba: image")
    slant = _slant(slant)
    if not math.isfinite(float(y)):
        raise ValueError(f"y {y!r}: expected a finite value")
    ctx = ctx or default_context()
    per_char = _per_char(text, color, colors)
    if len(text) == 0 or w == 0 or h == 0:
        return image
    line = placed_line(font, text, font_size, x, y, w, h, slant)
    if line is None:
        return image
    return _render(ctx, line, w, h, samples_per_axis, phase, _flags(flags | L.FR_TEXT_LOAD, srgb, bgra, cache, over),
                   colours=per_char, image=image)


def decoration_rects(font: Font, text, font_size: int, x: float, y: float, underline=None, strikeout=None, highlight=None):
    """The rectangles that decorate the line draw_text_rgba(image, font, text, font_size, x, y) draws, for RGBA.fill_rects /
    fr_layer_rects: rows of (x0, y0, x1, y1, (R, G, B, A)) in pixels, every edge an exact multiple of 1/64 (fill_rects
    takes them as they are, make_rects takes 64 times the edges), in drawing order: the highlight (the line box, ascender to descender), the underline, the strike-out, each for
    the colour given and left out for None.  x spans from the pen origin x64 = floor(64 x + 1/2) to x64 + the end pen; y
    is pen_y64 = floor(64 y + 1/2) plus the offsets of Font.decoration.  A highlight goes down before the text, the
    lines after it."""
    if not math.isfinite(float(x)) or not math.isfinite(float(y)):
        raise ValueError(f"x {x!r}, y {y!r}: expected finite values")
    _, _, end = font.layout(text, font_size)
    x64, y64 = q64(x), q64(y)
    rows = []
    for colour, kind in ((highlight, L.FR_DECOR_LINE_BOX), (underline, L.FR_DECOR_UNDERLINE), (strikeout, L.FR_DECOR_STRIKEOUT)):
        if colour is None:
            continue
        top, bottom = font.decoration(font_size, kind)
        rows.append((x64 / 64.0, (y64 + top) / 64.0, (x64 + end) / 64.0, (y64 + bottom) / 64.0, colour_rgba(colour)))
    return rows


def span_line(font: Font, spans):
    """Spans (text, font_size, slant, rise, colour) laid out as one line on a common baseline by chaining fr_text_layout:
    each span starts at the previous span's end pen (1/64 pixel where the size changes); rise: pixels above the baseline, kept to 1/64
    pixel (pen_y64 = baseline - floor(64 rise + 1/2)); every placement carries its span's scale f32(font_size) /
    f32(units_per_em) and slant.  -> (glyph set, fr_glyph_place_ex places, runs, width, height, per-character colours),
    or None when nothing is drawn.  One run; the image is the union of the instance cells, as for render_text."""
    spans = [tuple(sp) for sp in spans]
    for sp in spans:
        if len(sp) != 5:
            raise ValueError(f"span {sp!r}: expected (text, font_size, slant, rise, colour)")
        _, size, slant, rise, colour = sp
        if not isinstance(size, (int, np.integer)) or not 1 <= size <= 65535:
            raise ValueError(f"span font_size {size!r}: expected an integer in [1, 65535]")
        if not math.isfinite(float(rise)):
            raise ValueError(f"span rise {rise!r}: expected a finite value")
        _slant(slant), colour_rgba(colour)
    # consecutive spans of one size are one fr_text_layout call (the pen walks on unrounded, as inside one string, so
    # spans of a single size give exactly that string's pens); where the size changes the next call starts at the end pen
    glyphs, rows, colours, start, k = [], [], [], 0, 0
    while k < len(spans):
        m = k
        while m < len(spans) and spans[m][1] == spans[k][1]:
            m += 1
        texts = [[ord(c) for c in sp[0]] if isinstance(sp[0], str) else [int(c) for c in sp[0]] for sp in spans[k:m]]
        gi, pen, end = font.layout([c for t in texts for c in t], int(spans[k][1]))
        glyphs += list(gi)
        at = 0
        for t, (_, size, slant, rise, colour) in zip(texts, spans[k:m]):
            rows += [(int(p) + start, -q64(rise), _scale(font, size), _slant(slant)) for p in pen[at:at + len(t)]]
            colours += [colour_rgba(colour)] * len(t)
            at += len(t)
        start += end
        k = m
    if not glyphs:
        return None
    gs, local = _glyphs(font, glyphs)
    fit = _fit(gs, [(g,) + row for g, row in zip(local, rows)])
    return None if fit is None else (gs,) + fit + (colours,)


def render_spans(font: Font, spans, *, samples_per_axis: int = 4, mode: int = L.FR_COVERAGE_U8, phase: int = L.FR_SAMPLE_CENTER,
                 flags: int = 0, ctx: Optional[Context] = None) -> Gray:
    """One line made of spans (text, font_size, slant, rise, colour) — a heading word, a superscript, an oblique word
    inside an upright line — as one image from one run (span_line; the colours are not used here)."""
    line = span_line(font, spans)
    if line is None:
        return Gray.init(0, 0)
    return _render(ctx, line[:3], *line[3:5], samples_per_axis, phase, flags, mode)


def render_spans_rgba(font: Font, spans, background=(0, 0, 0, 0), *, samples_per_axis: int = 4, phase: int = L.FR_SAMPLE_CENTER,
                      flags: int = 0, srgb: bool = False, bgra: bool = False, over: bool = False,
                      ctx: Optional[Context] = None) -> RGBA:
    """render_spans as one RGBA image: every span's glyphs in its colour, blended per sample in order over `background`
    (srgb / bgra / over as render_text_rgba: with over the image is premultiplied)."""
    clear = colour_rgba(background)
    line = span_line(font, spans)
    if line is None:
        return RGBA.init(0, 0)
    return _render(ctx, line[:3], *line[3:5], samples_per_axis, phase, _flags(flags, srgb, bgra, over=over), colours=line[5],
                   clear=clear)


def view_line(font: Font, text, font_size: int, zoom: float, offset_x: float, offset_y: float, width: int, height: int,
              slant: float = 0.0):
    """The reference's frame (Appli.zig zoom / drag; shader.slang: position * transform.scale + transform.offset): the
    line laid out at `font_size`, then every position multiplied by `zoom` and moved by the offset, in pixels.  Glyph k's
    origin is at x = offset_x + zoom * pen_k and the baseline at y = offset_y, both kept to 1/64 pixel (floor(64 v +
    1/2)); the scale is f32(f32(font_size) * f32(zoom)) / f32(units_per_em).  -> (glyph set, fr_glyph_place_ex places,
    runs): one run of width x height pixels that clips the line, or None for an empty text or image."""
    zoom = _zoom(zoom)
    if not (math.isfinite(float(offset_x)) and math.isfinite(float(offset_y))):
        raise ValueError("offset_x / offset_y: expected finite values")
    _frame(width, height)
    slant = _slant(slant)
    laid = _layout(font, text, font_size, width == 0 or height == 0)
    if laid is None:
        return None
    gs, local, pens, _ = laid
    y64 = q64(offset_y)
    places = make_places_ex([(g, math.floor(64.0 * float(offset_x) + zoom * p + 0.5), y64, 0.0, slant) for g, p in zip(local, pens)])
    return gs, places, make_runs([(0, len(places), int(width), int(height), 0, 0, _scale(font, font_size, zoom))])


def render_text_view(font: Font, text, font_size: int, zoom: float, offset_x: float, offset_y: float, width: int, height: int,
                     *, slant: float = 0.0, samples_per_axis: int = 4, mode: int = L.FR_COVERAGE_U8,
                     phase: int = L.FR_SAMPLE_CENTER, flags: int = 0, ctx: Optional[Context] = None) -> Gray:
    """One frame of the reference's view: `text` at font_size * zoom with its origin at the fractional pixel position
    (offset_x, offset_y), clipped to a width x height image (view_line).  A slow zoom or drag moves the line by 1/64
    pixel in both axes."""
    line = view_line(font, text, font_size, zoom, offset_x, offset_y, width, height, slant)
    if line is None:
        return Gray.init(int(width), int(height))
    return _render(ctx, line, int(width), int(height), samples_per_axis, phase, flags, mode)


def _cos_sin(angle_deg: float):
    """cos and sin of an angle in degrees; at the quarter turns exactly 0 and +-1"""
    a = math.fmod(float(angle_deg), 360.0)
    if a == math.floor(a) and int(a) % 90 == 0:
        return ((1.0, 0.0), (0.0, 1.0), (-1.0, 0.0), (0.0, -1.0))[(int(a) // 90) % 4]
    r = math.radians(a)
    return math.cos(r), math.sin(r)


def rotated_line(font: Font, text, font_size: int, angle_deg: float, x: float, y: float, width: int, height: int,
                 zoom: float = 1.0, slant: float = 0.0):
    """A line along a direction: laid out at `font_size` by font.layout, its origin at the pixel position (x, y) (y
    downwards) and its baseline turned by angle_deg counter-clockwise.  Glyph k's pen is at (x + cos * zoom * pen_k / 64,
    y - sin * zoom * pen_k / 64), kept to 1/64 pixel (floor(64 v + 1/2)); every placement's matrix is
    s * R(angle) * [[1, slant], [0, 1]] with s = font_size * zoom / units_per_em, computed in binary64 and rounded once to
    binary32.  At the quarter turns cos and sin are exactly 0 and +-1, so those matrices are exact.  -> (glyph set,
    fr_glyph_place_affine places, runs): one run of width x height pixels that clips the line, or None for an empty text
    or image."""
    zoom = _zoom(zoom)
    if not (math.isfinite(float(x)) and math.isfinite(float(y)) and math.isfinite(float(angle_deg))):
        raise ValueError("x / y / angle_deg: expected finite values")
    _frame(width, height)
    k = _slant(slant)
    laid = _layout(font, text, font_size, width == 0 or height == 0)
    if laid is None:
        return None
    gs, local, pens, _ = laid
    c, sn = _cos_sin(angle_deg)
    s = float(font_size) * zoom / float(font.information.units_per_em)
    m = (s * c, s * (c * k - sn), s * sn, s * (sn * k + c))
    places = make_places_affine([(g, q64(float(x) + c * zoom * p / 64.0), q64(float(y) - sn * zoom * p / 64.0)) + m
                                 for g, p in zip(local, pens)])
    return gs, places, make_runs([(0, len(places), int(width), int(height), 0, 0, 1.0)])


def render_text_rotated(font: Font, text, font_size: int, angle_deg: float, x: float, y: float, width: int, height: int, *,
                        zoom: float = 1.0, slant: float = 0.0, samples_per_axis: int = 4, mode: int = L.FR_COVERAGE_U8,
                        phase: int = L.FR_SAMPLE_CENTER, flags: int = L.FR_FILL_CONSISTENT, cache: bool = False,
                        ctx: Optional[Context] = None) -> Gray:
    """`text` along a direction (rotated_line), clipped to a width x height image: a vertical axis title is angle_deg = 90
    with (x, y) at its lower end.  FR_FILL_CONSISTENT is the default here: under a rotation the reference's false
    windings on rows through vertices become slanted streaks (include/fr_raster.h).  cache: FR_TEXT_CACHE_AFFINE, the same
    bytes with each distinct (glyph, pen fractions, matrix) rasterised once per render; it pays when characters repeat
    at equal fractions and costs the mask store otherwise."""
    line = rotated_line(font, text, font_size, angle_deg, x, y, width, height, zoom, slant)
    if line is None:
        return Gray.init(int(width), int(height))
    return _render(ctx, line, int(width), int(height), samples_per_axis, phase, _flags(flags, cache=cache, affine=True), mode)


def render_text_rgba_rotated(font: Font, text, font_size: int, angle_deg: float, x: float, y: float, width: int, height: int,
                             color=(225, 105, 180, 255), background=(0, 0, 0, 0), colors=None, *, zoom: float = 1.0,
                             slant: float = 0.0, samples_per_axis: int = 4, phase: int = L.FR_SAMPLE_CENTER,
                             flags: int = L.FR_FILL_CONSISTENT, srgb: bool = False, bgra: bool = False, over: bool = False,
                             cache: bool = False, ctx: Optional[Context] = None) -> RGBA:
    """render_text_rotated as one RGBA image: colours, background, srgb, bgra and over as render_text_rgba (with over the
    image is premultiplied); cache as render_text_rotated"""
    per_char, clear = _per_char(text, color, colors), colour_rgba(background)
    line = rotated_line(font, text, font_size, angle_deg, x, y, width, height, zoom, slant)
    if line is None:
        im = RGBA.init(int(width), int(height))
        im.data[:] = clear
        return im
    return _render(ctx, line, int(width), int(height), samples_per_axis, phase, _flags(flags, srgb, bgra, cache, over, affine=True),
                   colours=per_char, clear=clear)


# ---- sub-pixel (LCD) text

def lcd_line(font: Font, text, font_size: int, x: float, y: float, width: int, height: int):
    """The line draw_text_lcd draws, as a coverage plane three times as wide as the image: laid out at `font_size` with the
    pen origin at image x and the baseline at image y, both kept to 1/64 pixel (floor(64 v + 1/2)), then stretched by 3
    along x: every placement's matrix is {3 s, 0, 0, s} with s = font_size / units_per_em, and its pen's x is 3 times
    the image's, in 1/64 plane element, so element 3 u + j of the plane is sub-pixel j of image pixel u.  -> (glyph set,
    fr_glyph_place_affine places, runs): one run of 3 width x height elements that clips the line, or None for an empty
    text or image."""
    if not (math.isfinite(float(x)) and math.isfinite(float(y))):
        raise ValueError("x / y: expected finite values")
    _frame(width, height)
    if 3 * int(width) > 65535:
        raise ValueError(f"width {width!r}: the plane of 3 x width elements must not be wider than 65535")
    laid = _layout(font, text, font_size, width == 0 or height == 0)
    if laid is None:
        return None
    gs, local, pens, _ = laid
    s = float(font_size) / float(font.information.units_per_em)
    x64, y64 = q64(x), q64(y)
    places = make_places_affine([(g, 3 * (x64 + p), y64, 3.0 * s, 0.0, 0.0, s) for g, p in zip(local, pens)])
    return gs, places, make_runs([(0, len(places), 3 * int(width), int(height), 0, 0, 1.0)])


def draw_text_lcd(image: RGBA, font: Font, text, font_size: int, x: float, y: float, color=(0, 0, 0, 255), *, weights=None,
                  samples_per_axis: int = 4, phase: int = L.FR_SAMPLE_CENTER, flags: int = L.FR_FILL_CONSISTENT,
                  srgb: bool = False, bgr: bool = False, return_plane: bool = False, cache: bool = False,
                  ctx: Optional[Context] = None):
    """One line of sub-pixel (LCD) text drawn in place over the premultiplied `image`: the line is rendered once as a
    coverage plane of 3 width x height elements through the affine text plan (lcd_line; 3 x samples_per_axis sample
    columns per pixel), and fr_layer_lcd filters it across sub-pixels with `weights` (None: the default filter) and
    composites `color` with an alpha per colour byte, both on the context's stream with no sync between them.  x, y as
    draw_text_rgba; the whole colour applies to the whole line.  srgb: the image is premultiplied in linear light; bgr:
    the panel's stripes are B G R.  FR_FILL_CONSISTENT is the default, as for rotated text.  cache: FR_TEXT_CACHE_AFFINE
    for the plane's plan: the same plane, each distinct (glyph, pen fraction) of the line rasterised once.  Returns
    `image`, or (image, the plane as a Gray) with return_plane."""
    w, h = image.width, image.height
    dst = rgba_pixels(image, "draw_text_lcd: image")
    colour = colour_rgba(color)
    ctx = ctx or default_context()
    line = None if len(text) == 0 else lcd_line(font, text, font_size, x, y, w, h)
    if line is None:
        return (image, Gray.init(3 * w, h)) if return_plane else image
    gs, places, runs = line
    blits = make_lcd_blits([(0, 0, w, h, 0, 0, colour)])
    with closing(DeviceGlyphSet(ctx, gs)) as dgs, closing(TextPlan(dgs, places, runs, L.FR_COVERAGE_U8, samples_per_axis, phase,
                                                                 _flags(flags, cache=cache, affine=True))) as plan:
        def call(d, c):
            plan.render(c, 3 * w, h)
            layer_lcd(ctx, c, 3 * w, h, d, w, h, blits, weights, srgb, bgr)
        out, cov = round_trip(ctx, call, dst, (h * 3 * w,), back=(0, 1))
    image.data[:] = out
    return (image, Gray(3 * w, h, cov)) if return_plane else image


def render_text_lcd(font: Font, text, font_size: int, x: float, y: float, width: int, height: int, color=(0, 0, 0, 255),
                    background=(255, 255, 255, 255), *, weights=None, samples_per_axis: int = 4, phase: int = L.FR_SAMPLE_CENTER,
                    flags: int = L.FR_FILL_CONSISTENT, srgb: bool = False, bgr: bool = False, cache: bool = False,
                    ctx: Optional[Context] = None) -> RGBA:
    """draw_text_lcd over a new width x height image filled with the premultiplied colour `background`: black text on
    white by default, what sub-pixel rendering is made for; cache as draw_text_lcd"""
    _frame(width, height)
    im = RGBA.init(int(width), int(height))
    im.data[:] = colour_rgba(background)
    return draw_text_lcd(im, font, text, font_size, x, y, color, weights=weights, samples_per_axis=samples_per_axis, phase=phase,
                         flags=flags, srgb=srgb, bgr=bgr, cache=cache, ctx=ctx)

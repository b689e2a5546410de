"""Text runs: a string laid out by the reference's pen walk (Appli.zig:318-349) and rendered as one anti-aliased image
through a text plan (fr_text_plan_create, include/fr_raster.h), or as one RGBA image through an RGBA text plan
(fr_text_plan_create_rgba), or drawn over an RGBA image the caller has (FR_TEXT_LOAD).  Nothing is computed in Python but
the image size and the pen positions."""
from __future__ import annotations

import math
from typing import Optional

import numpy as np

from . import _lib as L
from .font import Font
from .image import RGBA, Gray
from .render_glyph import Context, DeviceGlyphSet, TextPlan, TextPlanRGBA, default_context, make_places, make_runs


def instance_cell(box, scale: float, pen_x64: int, pen_y: int):
    """an instance's cell in image coordinates, unclipped -> (column 0, row 0, width, height): renderGlyph's grid at
    `scale` (binary32 as render_glyph.zig:13-17), one column wider when the pen has a fractional part"""
    s = np.float32(scale)
    b = np.asarray(box, np.int16).astype(np.float32) * s
    mn_x, mn_y = math.floor(b[0]), math.floor(b[1])
    mx_x, mx_y = math.ceil(b[2]), math.ceil(b[3])
    ix, fx64 = pen_x64 >> 6, pen_x64 & 63
    return ix + mn_x, pen_y - mx_y, mx_x - mn_x + 1 + (fx64 != 0), mx_y - mn_y + 1


def _line(font: Font, text, font_size: int):
    """one line laid out as one run: (glyph set, places, runs, width, height), or None when nothing is drawn.  The image
    is the union of the instance cells: the pen origin at its left edge (moved right by whole pixels if a cell reaches
    left of it) and the baseline at row ceil(max y_max * scale)."""
    gi, pen, _ = font.layout(text, font_size)
    distinct = sorted(set(int(g) for g in gi))
    gs, kept = font.glyphset(distinct, skip_unsupported=False)
    local = {g: k for k, g in enumerate(kept)}
    scale = np.float32(font_size) / np.float32(font.information.units_per_em)
    cells = [instance_cell(gs.boxes[local[int(g)]], scale, int(p), 0) for g, p in zip(gi, pen)
             if gs.segments_per_glyph()[local[int(g)]] > 0]
    if not cells:
        return None
    left = min(c[0] for c in cells)
    shift = -left if left < 0 else 0                       # whole pixels: the fractional pens stay as laid out
    top = min(c[1] for c in cells)                         # the baseline row is -top = ceil(max y_max * scale)
    width = max(c[0] + c[2] for c in cells) + shift
    height = max(c[1] + c[3] for c in cells) - top
    places = make_places([(local[int(g)], int(p) + 64 * shift, -top) for g, p in zip(gi, pen)])
    runs = make_runs([(0, len(places), width, height, 0, 0, scale)])
    return gs, places, runs, width, height


def render_text(font: Font, text, font_size: int, *, samples_per_axis: int = 4, mode: int = L.FR_COVERAGE_U8,
                phase: int = L.FR_SAMPLE_CENTER, flags: int = 0, ctx: Optional[Context] = None) -> Gray:
    """One line of text as one image: every glyph at its sub-pixel pen, overlapping glyphs unioned per sample.
    The image is the union of the instance cells: the pen origin at its left edge (moved right by whole pixels if a cell
    reaches left of it) and the baseline at row ceil(max y_max * scale)."""
    import torch

    ctx = ctx or default_context()
    line = _line(font, text, font_size)
    if line is None:
        return Gray.init(0, 0)
    gs, places, runs, width, height = line
    dgs = DeviceGlyphSet(ctx, gs)
    plan = TextPlan(dgs, places, runs, mode, samples_per_axis, phase, flags)
    try:
        buf = torch.empty((height, width), dtype=torch.uint8, device=f"cuda:{ctx.device}")
        torch.cuda.synchronize(ctx.device)
        plan.render(buf.data_ptr(), width, height)
        ctx.sync()
        im = Gray.init(width, height)
        im.data[:] = buf.cpu().numpy().reshape(-1)
    finally:
        plan.close()
        dgs.close()
    return im


def _rgba(c) -> tuple:
    """an (R, G, B) or (R, G, B, A) colour -> (R, G, B, A), A = 255 when omitted"""
    c = tuple(int(v) for v in c)
    if len(c) == 3:
        c += (255,)
    if len(c) != 4 or not all(0 <= v <= 255 for v in c):
        raise ValueError(f"colour {c}: expected 3 or 4 values in [0, 255]")
    return c


def render_text_rgba(font: Font, text, font_size: int, color=(225, 105, 180, 255), background=(0, 0, 0, 0), colors=None,
                     *, samples_per_axis: int = 4, phase: int = L.FR_SAMPLE_CENTER, flags: int = 0, srgb: bool = False,
                     bgra: bool = False, ctx: Optional[Context] = None) -> RGBA:
    """One line of text as one RGBA image (fr_text_plan_create_rgba): every glyph blended per sample in order over
    `background`, in `color` or, if `colors` is given, in colors[k] for character k (e.g. to highlight a word).  The
    defaults are the reference's frame: pink text (shader.slang) on a transparent clear colour.  Sized as render_text.
    srgb: blend and resolve in linear light, as the reference's sRGB swapchain does (FR_TEXT_SRGB); bgra: the pixels'
    bytes are B G R A (FR_TEXT_BGRA; the colours stay R G B A)."""
    import torch

    ctx = ctx or default_context()
    flags |= (L.FR_TEXT_SRGB if srgb else 0) | (L.FR_TEXT_BGRA if bgra else 0)
    n_chars = len(text)
    if colors is not None and len(colors) != n_chars:
        raise ValueError(f"colors: {len(colors)} colours for {n_chars} characters")
    per_char = [_rgba(c) for c in colors] if colors is not None else [_rgba(color)] * n_chars
    clear = _rgba(background)
    line = _line(font, text, font_size)
    if line is None:
        return RGBA.init(0, 0)
    gs, places, runs, width, height = line
    dgs = DeviceGlyphSet(ctx, gs)
    plan = TextPlanRGBA(dgs, places, per_char, runs, [clear], samples_per_axis, phase, flags)
    try:
        buf = torch.empty((height, width, 4), dtype=torch.uint8, device=f"cuda:{ctx.device}")
        torch.cuda.synchronize(ctx.device)
        plan.render(buf.data_ptr(), width, height)
        ctx.sync()
        im = RGBA.init(width, height)
        im.data[:] = buf.cpu().numpy().reshape(-1, 4)
    finally:
        plan.close()
        dgs.close()
    return im


def draw_text_rgba(image: RGBA, font: Font, text, font_size: int, x: float, y: int, color=(225, 105, 180, 255), colors=None,
                   *, samples_per_axis: int = 4, phase: int = L.FR_SAMPLE_CENTER, flags: int = 0, srgb: bool = False,
                   bgra: bool = False, ctx: Optional[Context] = None) -> RGBA:
    """One line of text drawn in place into `image` (FR_TEXT_LOAD): every sample starts at the pixel already there, and
    the glyphs are blended over it per sample in order, in `color` or colors[k] for character k.  x: the pen origin's
    image x in pixels (fractional x is kept to 1/64 pixel: pen_x64 = floor(64 x + 1/2)); y: the baseline's row.  The
    line is one run covering the whole image, so glyphs are clipped at its edges.  The whole image is copied to the
    device and back; on the device only the 64 x 16 tiles that some glyph cell meets are read (and, where needed,
    written), and every pixel no glyph sample reaches comes back with its bytes unchanged.  srgb / bgra as
    render_text_rgba: the image's bytes are sRGB / B G R A.  image.data must be a (height * width, 4) uint8 array
    (ValueError otherwise).  Returns `image`."""
    import torch

    w, h, data = image.width, image.height, image.data
    if not (isinstance(w, (int, np.integer)) and isinstance(h, (int, np.integer)) and w >= 0 and h >= 0):
        raise ValueError(f"image: width {w!r} and height {h!r} must be non-negative integers")
    if not isinstance(data, np.ndarray) or data.dtype != np.uint8 or data.shape != (h * w, 4):
        raise ValueError(f"image.data: expected a ({h * w}, 4) uint8 array for {w} x {h} pixels, got "
                         f"{getattr(data, 'shape', None)} {getattr(data, 'dtype', type(data).__name__)}")
    ctx = ctx or default_context()
    flags |= L.FR_TEXT_LOAD | (L.FR_TEXT_SRGB if srgb else 0) | (L.FR_TEXT_BGRA if bgra else 0)
    n_chars = len(text)
    if colors is not None and len(colors) != n_chars:
        raise ValueError(f"colors: {len(colors)} colours for {n_chars} characters")
    per_char = [_rgba(c) for c in colors] if colors is not None else [_rgba(color)] * n_chars
    if n_chars == 0 or image.width == 0 or image.height == 0:
        return image
    gi, pen, _ = font.layout(text, font_size)
    gs, kept = font.glyphset(sorted(set(int(g) for g in gi)), skip_unsupported=False)
    local = {g: k for k, g in enumerate(kept)}
    scale = np.float32(font_size) / np.float32(font.information.units_per_em)
    x64 = math.floor(64.0 * float(x) + 0.5)
    places = make_places([(local[int(g)], x64 + int(p), int(y)) for g, p in zip(gi, pen)])
    runs = make_runs([(0, len(places), image.width, image.height, 0, 0, scale)])
    dgs = DeviceGlyphSet(ctx, gs)
    try:
        plan = TextPlanRGBA(dgs, places, per_char, runs, None, samples_per_axis, phase, flags)
        try:
            buf = torch.from_numpy(np.ascontiguousarray(image.data)).to(f"cuda:{ctx.device}")
            torch.cuda.synchronize(ctx.device)
            plan.render(buf.data_ptr(), image.width, image.height)
            ctx.sync()
            image.data[:] = buf.cpu().numpy()
        finally:
            plan.close()
    finally:
        dgs.close()
    return image

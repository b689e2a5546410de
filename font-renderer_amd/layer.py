"""The layer calls of the C ABI (fr_layer_*, include/fr_raster.h) on device addresses, and the builders of their tables.
All of them are asynchronous on the context's stream; RGBA.over / blend / over_warped / over_masked / erase / fill_rects / paint / draw_lcd / shadow / outline / unpremultiply
(image.py) wrap them for host images."""
from __future__ import annotations

import ctypes as C
import math
from fractions import Fraction
from typing import Sequence

import numpy as np

from . import _lib as L
from .device import Context

BLIT_DTYPE = np.dtype(L.LayerBlit)
RECT_DTYPE = np.dtype(L.LayerRect)
LCD_BLIT_DTYPE = np.dtype(L.LcdBlit)
MASK_BLIT_DTYPE = np.dtype(L.LayerMaskBlit)
WARP_BLIT_DTYPE = np.dtype(L.LayerWarpBlit)


def make_blits(rows: Sequence) -> np.ndarray:
    """rows of (src_x, src_y, w, h, dst_x, dst_y, opacity) -> fr_layer_blit array"""
    return np.array([tuple(r) for r in rows], BLIT_DTYPE)


def make_mask_blits(rows: Sequence) -> np.ndarray:
    """rows of (src_x, src_y, w, h, dst_x, dst_y, mask_x, mask_y, opacity, invert) -> fr_layer_mask_blit array"""
    return np.array([tuple(r) for r in rows], MASK_BLIT_DTYPE)


def make_warp_blits(rows: Sequence) -> np.ndarray:
    """rows of (src_x, src_y, w, h, dst_x, dst_y, dst_w, dst_h, u0, v0, ux, uy, vx, vy, opacity[, reserved]) -> fr_layer_warp_blit
    array: the window of the layer, the rectangle of the image, and the inverse map in 1/65536 window pixel"""
    return np.array([tuple(int(v) for v in r) + (0,) * (16 - len(r)) for r in rows], WARP_BLIT_DTYPE)


def warp_from_matrix(matrix, window, opacity: int = 255) -> tuple:
    """The fr_layer_warp_blit row (for make_warp_blits) that places the window = (src_x, src_y, w, h) of a layer through the
    forward map `matrix` = ((a, b, tx), (c, d, ty)): the point (u, v) of the window, in pixels with pixel centres at + 1/2,
    lands on (a u + b v + tx, c u + d v + ty) of the image, pixel centres at + 1/2 there too.  The matrix is inverted in
    exact rationals (floats are taken at their exact value) and each coefficient of the inverse map rounded as
    floor(65536 x + 1/2).  The blit's rectangle is the bounding box of the image of [-1/2, w + 1/2] x [-1/2, h + 1/2], every
    point a tap can reach, grown by one pixel all round.  ValueError: a singular matrix, or a map beyond the call's ranges."""
    (a, b, tx), (c, d, ty) = [[Fraction(v) for v in row] for row in matrix]
    sx, sy, w, h = (int(v) for v in window)
    det = a * d - b * c
    if det == 0:
        raise ValueError(f"matrix {matrix!r} is singular")
    half = Fraction(1, 2)
    corners = [(a * u + b * v + tx, c * u + d * v + ty) for u in (-half, w + half) for v in (-half, h + half)]
    x0, y0 = math.floor(min(p[0] for p in corners)) - 1, math.floor(min(p[1] for p in corners)) - 1
    x1, y1 = math.ceil(max(p[0] for p in corners)) + 1, math.ceil(max(p[1] for p in corners)) + 1
    ia, ib, ic, id_ = d / det, -b / det, -c / det, a / det
    q = lambda v: math.floor(65536 * v + half)
    cx, cy = x0 + half - tx, y0 + half - ty                  # the centre of rectangle pixel (0, 0), from the map's origin
    row = (sx, sy, w, h, x0, y0, x1 - x0, y1 - y0, q(ia * cx + ib * cy), q(ic * cx + id_ * cy), q(ia), q(ib), q(ic), q(id_), int(opacity))
    if not (all(-2 ** 31 <= v < 2 ** 31 for v in row[4:6] + row[10:14]) and all(abs(v) <= 2 ** 47 for v in row[8:10]) and all(v <= 2 ** 26 for v in row[6:8])):
        raise ValueError(f"matrix {matrix!r} over a window of {w} x {h}: beyond the ranges of fr_layer_warp")
    return row


def make_rects(rows: Sequence) -> np.ndarray:
    """rows of (x0, y0, x1, y1, (R, G, B, A)), the edges in 1/64 pixel -> fr_layer_rect array"""
    return np.array([(int(r[0]), int(r[1]), int(r[2]), int(r[3]), tuple(int(v) for v in r[4])) for r in rows], RECT_DTYPE)


def make_lcd_blits(rows: Sequence) -> np.ndarray:
    """rows of (src_x, src_y, w, h, dst_x, dst_y, (R, G, B, A)) -> fr_lcd_blit array: src_x in plane elements (three per
    pixel), w and h in destination pixels, the colour straight"""
    return np.array([tuple(int(v) for v in r[:6]) + (tuple(int(v) for v in r[6]),) for r in rows], LCD_BLIT_DTYPE)


def _gradient(kind: int, geometry, stops, spread: int) -> L.LayerPaintParams:
    stops = [(int(off), tuple(int(v) for v in rgba)) for off, rgba in stops]
    if not 1 <= len(stops) <= L.FR_GRADIENT_MAX_STOPS:
        raise ValueError(f"{len(stops)} gradient stops: expected 1 .. {L.FR_GRADIENT_MAX_STOPS}")
    if not all(0 <= off < 2 ** 32 and len(rgba) == 4 and all(0 <= v <= 255 for v in rgba) for off, rgba in stops):
        raise ValueError(f"gradient stops {stops!r}: expected (offset, (R, G, B, A)) with bytes in [0, 255]")
    if not all(-2 ** 31 <= int(v) < 2 ** 31 for v in geometry):
        raise ValueError(f"gradient geometry {tuple(geometry)!r}: a value beyond int32 in 1/64 pixel")
    p = L.LayerPaintParams(kind=kind, spread=int(spread), n_stops=len(stops))
    p.x0, p.y0, p.x1, p.y1 = (int(v) for v in geometry)
    for i, (off, rgba) in enumerate(stops):
        p.stops[i] = L.GradientStop(off, (C.c_uint8 * 4)(*rgba))
    return p


def make_gradient_linear(x0: int, y0: int, x1: int, y1: int, stops, spread: int = L.FR_SPREAD_PAD) -> L.LayerPaintParams:
    """a linear gradient from (x0, y0) to (x1, y1), in 1/64 pixel of the destination image, y down -> the gradient part of
    an fr_layer_paint_params (layer_paint fills in the window and the position).  stops: 1 .. 8 of (offset, (R, G, B, A)),
    offset in 0 .. 65536 and not decreasing, the colour straight; spread: FR_SPREAD_PAD, _REPEAT or _REFLECT."""
    return _gradient(L.FR_GRADIENT_LINEAR, (x0, y0, x1, y1), stops, spread)


def make_gradient_radial(cx: int, cy: int, r: int, stops, spread: int = L.FR_SPREAD_PAD) -> L.LayerPaintParams:
    """a radial gradient around (cx, cy) that reaches offset 65536 at radius r, in 1/64 pixel of the destination image
    -> the gradient part of an fr_layer_paint_params; stops and spread as for make_gradient_linear"""
    return _gradient(L.FR_GRADIENT_RADIAL, (cx, cy, r, 0), stops, spread)


def _table(rows, dtype):
    """an optional table -> (C-contiguous array or None, row count)"""
    return (None, 0) if rows is None else (np.ascontiguousarray(rows, dtype), len(rows))


def _flags(flags: int, srgb: bool) -> int:
    return flags | (L.FR_LAYER_SRGB if srgb else 0)


def layer_over(ctx: Context, src_ptr: int, src_stride_px: int, src_rows: int, dst_ptr: int, dst_stride_px: int, dst_rows: int,
               blits, srgb: bool = False, flags: int = 0) -> None:
    """fr_layer_over: rectangles of the premultiplied layer at device address src_ptr composited over the premultiplied
    image at dst_ptr (both 4 bytes per pixel, alpha last; strides and rows in pixels), asynchronous on the context's
    stream.  blits: an fr_layer_blit array (make_blits) or None.  srgb: FR_LAYER_SRGB, composite in linear light."""
    b, n = _table(blits, BLIT_DTYPE)
    L.check(ctx._lib.fr_layer_over(ctx._h, C.c_void_p(src_ptr), src_stride_px, src_rows, C.c_void_p(dst_ptr), dst_stride_px,
                                   dst_rows, None if b is None else L.ptr(b), n, _flags(flags, srgb)))


def layer_rects(ctx: Context, dst_ptr: int, dst_stride_px: int, dst_rows: int, rects, srgb: bool = False, flags: int = 0) -> None:
    """fr_layer_rects: anti-aliased rectangles, each in one straight colour, composited in order over the premultiplied
    image at device address dst_ptr (4 bytes per pixel, alpha last; stride and rows in pixels), asynchronous on the
    context's stream.  rects: an fr_layer_rect array (make_rects) or None.  srgb: FR_LAYER_SRGB, composite in linear light."""
    r, n = _table(rects, RECT_DTYPE)
    L.check(ctx._lib.fr_layer_rects(ctx._h, C.c_void_p(dst_ptr), dst_stride_px, dst_rows, None if r is None else L.ptr(r), n,
                                    _flags(flags, srgb)))


def layer_paint(ctx: Context, src_ptr, src_stride_px: int, src_rows: int, dst_ptr: int, dst_stride_px: int, dst_rows: int,
                gradient, window, dst=(0, 0), srgb: bool = False, flags: int = 0) -> None:
    """fr_layer_paint: `gradient` (make_gradient_linear / make_gradient_radial) composited over the premultiplied image at
    device address dst_ptr through the alpha of the window = (src_x, src_y, w, h) of the layer at src_ptr, with the window's
    top-left pixel at dst = (dst_x, dst_y); src_ptr None or 0 (with src_stride_px = src_rows = 0 and a window at (0, 0)):
    full coverage, a gradient panel of w x h.  Strides and rows in pixels; asynchronous on the context's stream.  srgb:
    FR_LAYER_SRGB, composite in linear light.  gradient None passes a NULL parameter block (refused)."""
    p = None
    if gradient is not None:
        p = L.LayerPaintParams.from_buffer_copy(gradient)           # the caller's gradient stays as it is
        p.src_x, p.src_y, p.w, p.h = (int(v) for v in window)
        p.dst_x, p.dst_y = int(dst[0]), int(dst[1])
    L.check(ctx._lib.fr_layer_paint(ctx._h, C.c_void_p(src_ptr or None), src_stride_px, src_rows, C.c_void_p(dst_ptr), dst_stride_px, dst_rows,
                                    None if p is None else C.byref(p), _flags(flags, srgb)))


def layer_lcd(ctx: Context, cov_ptr: int, cov_stride: int, cov_rows: int, dst_ptr: int, dst_stride_px: int, dst_rows: int, blits,
              weights=None, srgb: bool = False, bgr: bool = False, flags: int = 0) -> None:
    """fr_layer_lcd: sub-pixel (LCD) text.  Windows of the coverage plane at device address cov_ptr (one byte per element,
    three elements per pixel, rows of cov_stride bytes) filtered across sub-pixels and composited over the premultiplied
    image at dst_ptr (4 bytes per pixel, alpha last; stride and rows in pixels) with one alpha per colour byte;
    asynchronous on the context's stream.  blits: an fr_lcd_blit array (make_lcd_blits) or None.  weights: FR_LCD_TAPS
    values that add up to 256, or None for the default (8, 77, 86, 77, 8).  srgb: FR_LAYER_SRGB, composite in linear light;
    bgr: FR_LCD_BGR, the panel's stripes are B G R (memory byte b takes sub-pixel 2 - b)."""
    b, n = _table(blits, LCD_BLIT_DTYPE)
    w = None
    if weights is not None:
        w = [int(v) for v in weights]
        if len(w) != L.FR_LCD_TAPS or not all(0 <= v <= 65535 for v in w):
            raise ValueError(f"weights {weights!r}: expected {L.FR_LCD_TAPS} values in [0, 65535]")
        w = (C.c_uint16 * L.FR_LCD_TAPS)(*w)
    L.check(ctx._lib.fr_layer_lcd(ctx._h, C.c_void_p(cov_ptr), cov_stride, cov_rows, C.c_void_p(dst_ptr), dst_stride_px, dst_rows,
                                  None if b is None else L.ptr(b), n, w, _flags(flags, srgb) | (L.FR_LCD_BGR if bgr else 0)))


def layer_mask(ctx: Context, src_ptr, src_stride_px: int, src_rows: int, mask_ptr: int, mask_stride: int, mask_rows: int, dst_ptr: int,
               dst_stride_px: int, dst_rows: int, blits, srgb: bool = False, plane: bool = False, erase: bool = False, flags: int = 0) -> None:
    """fr_layer_mask: fr_layer_over with an opacity per pixel.  Rectangles of the premultiplied layer at device address src_ptr
    composited over the premultiplied image at dst_ptr at t = m(k', opacity), where k is the alpha byte of the pixel of the
    layer at mask_ptr that lies over the pixel (4 bytes per pixel, mask_stride in pixels) and k' = 255 - k where the blit
    inverts; asynchronous on the context's stream.  blits: an fr_layer_mask_blit array (make_mask_blits) or None.  srgb:
    FR_LAYER_SRGB, composite in linear light.  plane: FR_MASK_PLANE, the mask is a plane of bytes (a coverage render;
    mask_stride in bytes, any alignment).  erase: FR_MASK_ERASE, no layer (src_ptr None or 0; src_stride_px and src_rows are
    ignored): the image is multiplied by 255 - t."""
    b, n = _table(blits, MASK_BLIT_DTYPE)
    L.check(ctx._lib.fr_layer_mask(ctx._h, C.c_void_p(src_ptr or None), src_stride_px, src_rows, C.c_void_p(mask_ptr), mask_stride, mask_rows,
                                   C.c_void_p(dst_ptr), dst_stride_px, dst_rows, None if b is None else L.ptr(b), n,
                                   _flags(flags, srgb) | (L.FR_MASK_PLANE if plane else 0) | (L.FR_MASK_ERASE if erase else 0)))


def layer_warp(ctx: Context, src_ptr: int, src_stride_px: int, src_rows: int, dst_ptr: int, dst_stride_px: int, dst_rows: int,
               blits, srgb: bool = False, flags: int = 0) -> None:
    """fr_layer_warp: windows of the premultiplied layer at device address src_ptr composited over the premultiplied image at
    dst_ptr through an affine map each, scaled, turned or moved by a fraction of a pixel, sampled bilinearly in exact
    integers (both 4 bytes per pixel, alpha last; strides and rows in pixels); asynchronous on the context's stream.
    blits: an fr_layer_warp_blit array (make_warp_blits; warp_from_matrix makes a row from a forward matrix) or None.
    srgb: FR_LAYER_SRGB, sample and composite in linear light."""
    b, n = _table(blits, WARP_BLIT_DTYPE)
    L.check(ctx._lib.fr_layer_warp(ctx._h, C.c_void_p(src_ptr), src_stride_px, src_rows, C.c_void_p(dst_ptr), dst_stride_px,
                                   dst_rows, None if b is None else L.ptr(b), n, _flags(flags, srgb)))


def layer_blend(ctx: Context, src_ptr: int, src_stride_px: int, src_rows: int, dst_ptr: int, dst_stride_px: int, dst_rows: int,
                blits, mode: int, srgb: bool = False, flags: int = 0) -> None:
    """fr_layer_blend: fr_layer_over with a blend mode in the place of source-over.  Rectangles of the premultiplied layer at
    device address src_ptr blended into the premultiplied image at dst_ptr (both 4 bytes per pixel, alpha last; strides and
    rows in pixels) in `mode`, one of FR_BLEND_MULTIPLY, _SCREEN, _OVERLAY, _DARKEN, _LIGHTEN, _HARD_LIGHT, _DIFFERENCE,
    _EXCLUSION and _PLUS; asynchronous on the context's stream.  blits: an fr_layer_blit array (make_blits) or None.  srgb:
    FR_LAYER_SRGB, blend in linear light."""
    b, n = _table(blits, BLIT_DTYPE)
    L.check(ctx._lib.fr_layer_blend(ctx._h, C.c_void_p(src_ptr), src_stride_px, src_rows, C.c_void_p(dst_ptr), dst_stride_px,
                                    dst_rows, None if b is None else L.ptr(b), n, mode, _flags(flags, srgb)))


def layer_unpremultiply(ctx: Context, ptr: int, stride_px: int, w: int, h: int, srgb: bool = False) -> None:
    """fr_layer_unpremultiply: the w x h window at device address ptr of an image with rows of stride_px pixels from
    premultiplied to straight alpha, in place, asynchronous on the context's stream"""
    L.check(ctx._lib.fr_layer_unpremultiply(ctx._h, C.c_void_p(ptr), stride_px, w, h, 1 if srgb else 0))


def layer_shadow(ctx: Context, src_ptr: int, src_stride_px: int, src_rows: int, dst_ptr: int, dst_stride_px: int, dst_rows: int,
                 window, rect, offset=(0, 0), spread: int = 0, blur_radius: int = 0, blur_passes: int = 0,
                 rgba=(0, 0, 0, 255), srgb: bool = False, flags: int = 0) -> None:
    """fr_layer_shadow: the alpha of the window (src_x, src_y, w, h) of the premultiplied layer at device address src_ptr,
    spread by a square maximum of radius `spread`, blurred by `blur_passes` box passes of radius `blur_radius`, moved by
    offset = (dx, dy) whole pixels and tinted with the straight colour rgba, written as a premultiplied R G B A layer over
    every pixel of rect = (dst_x, dst_y, dst_w, dst_h) of the image at dst_ptr (strides and rows in pixels); asynchronous
    on the context's stream.  srgb: FR_LAYER_SRGB, the colour bytes as an srgb=True render writes them.  window or rect
    None passes a NULL parameter block (refused)."""
    p = None
    if window is not None and rect is not None:
        p = L.LayerShadowParams(*[int(v) for v in window], *[int(v) for v in rect], int(offset[0]), int(offset[1]), int(spread),
                                int(blur_radius), int(blur_passes), (C.c_uint8 * 4)(*[int(v) for v in rgba]))
    L.check(ctx._lib.fr_layer_shadow(ctx._h, C.c_void_p(src_ptr), src_stride_px, src_rows, C.c_void_p(dst_ptr), dst_stride_px, dst_rows,
                                     None if p is None else C.byref(p), _flags(flags, srgb)))


def layer_outline(ctx: Context, src_ptr: int, src_stride_px: int, src_rows: int, dst_ptr: int, dst_stride_px: int, dst_rows: int,
                  window, rect, offset=(0, 0), radius: int = 16, kind: int = L.FR_OUTLINE_GROW, rgba=(0, 0, 0, 255),
                  srgb: bool = False, flags: int = 0) -> None:
    """fr_layer_outline: the alpha of the window (src_x, src_y, w, h) of the premultiplied layer at device address src_ptr,
    grown or shrunk by a disc of `radius` sixteenths of a pixel (0 .. FR_OUTLINE_MAX_RADIUS) as `kind` says (FR_OUTLINE_GROW:
    the grown shape, _RING: grown minus the layer, _INNER: the layer minus its shrunk shape, _SHRINK: the shrunk shape), moved
    by offset = (dx, dy) whole pixels and tinted with the straight colour rgba, written as a premultiplied R G B A layer over
    every pixel of rect = (dst_x, dst_y, dst_w, dst_h) of the image at dst_ptr (strides and rows in pixels); asynchronous
    on the context's stream.  srgb: FR_LAYER_SRGB, the colour bytes as an srgb=True render writes them.  window or rect
    None passes a NULL parameter block (refused)."""
    p = None
    if window is not None and rect is not None:
        p = L.LayerOutlineParams(*[int(v) for v in window], *[int(v) for v in rect], int(offset[0]), int(offset[1]), int(radius), int(kind),
                                 (C.c_uint8 * 4)(*[int(v) for v in rgba]))
    L.check(ctx._lib.fr_layer_outline(ctx._h, C.c_void_p(src_ptr), src_stride_px, src_rows, C.c_void_p(dst_ptr), dst_stride_px, dst_rows,
                                      None if p is None else C.byref(p), _flags(flags, srgb)))

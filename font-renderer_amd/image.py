"""Image sinks — mirror of /root/reference/src/tools/Image.zig:44-130 (Gray, Winding).
Row-major `data[y*width + x]`; getRGBLinear reproduces the reference's colour maps."""
from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np

from . import _lib as L
from .device import default_context, round_trip
from .glyph import GlyphSet
from .layer import (layer_blend, layer_lcd, layer_mask, layer_outline, layer_over, layer_paint, layer_rects, layer_shadow, layer_unpremultiply, layer_warp, make_blits, make_lcd_blits,
                    make_mask_blits, make_rects, make_warp_blits, warp_from_matrix)


def q64(v) -> int:
    """a pixel coordinate kept to 1/64 pixel, half up"""
    return math.floor(64.0 * float(v) + 0.5)


def colour_rgba(c, alpha_optional: bool = True) -> tuple:
    """an (R, G, B, A) colour, or (R, G, B) where the alpha is optional -> (R, G, B, A), A = 255 when omitted"""
    c = tuple(int(v) for v in c)
    if alpha_optional and len(c) == 3:
        c += (255,)
    if len(c) != 4 or not all(0 <= v <= 255 for v in c):
        raise ValueError(f"colour {c}: expected {'3 or 4' if alpha_optional else '4'} values in [0, 255]")
    return c


def rgba_pixels(image, what: str, sized: bool = True) -> np.ndarray:
    """the pixels of an RGBA image as a C-contiguous array; ValueError unless image.data is an (n, 4) uint8 array, with
    n = width * height when `sized`.  what: the caller's name for the image, for the message."""
    d, n = image.data, image.width * image.height
    if (not isinstance(d, np.ndarray) or d.dtype != np.uint8 or d.ndim != 2 or d.shape[1] != 4 or (sized and d.shape[0] != n)):
        raise ValueError(f"{what}: data must be a ({n if sized else 'n'}, 4) uint8 array"
                         + (f" for {image.width} x {image.height} pixels" if sized else "")
                         + f", got {getattr(d, 'shape', None)} {getattr(d, 'dtype', type(d).__name__)}")
    return np.ascontiguousarray(d)


@dataclass
class Gray:                     # Image.zig:44-83
    width: int
    height: int
    data: np.ndarray            # (height*width,) u8

    @staticmethod
    def init(width: int, height: int) -> "Gray":            # Image.zig:58-61
        return Gray(width, height, np.zeros(width * height, np.uint8))

    def getWidth(self) -> int:
        return self.width

    def getHeight(self) -> int:
        return self.height

    def getRGBLinear(self, index: int):                     # Image.zig:78-82
        v = int(self.data[index])
        return (v, v, v)

    def as_2d(self) -> np.ndarray:
        return self.data.reshape(self.height, self.width)


@dataclass
class Winding:                  # Image.zig:85-130
    width: int
    height: int
    data: np.ndarray            # (height*width,) i16
    scaler: int = 50
    overflow_color: int = 150

    @staticmethod
    def init(width: int, height: int, scaler: int, overflow_color: int) -> "Winding":   # Image.zig:101-104
        return Winding(width, height, np.zeros(width * height, np.int16), scaler, overflow_color)

    def getWidth(self) -> int:
        return self.width

    def getHeight(self) -> int:
        return self.height

    def getRGBLinear(self, index: int):                     # Image.zig:121-129
        val = int(self.data[index])
        if val == 0:
            return (0, 0, 0)
        c = min(self.scaler * abs(val), 65535)              # u16 saturating multiply
        color = min(c, 255)
        sub = 0 if c == color else self.overflow_color
        return (sub, sub, color) if val > 0 else (color, sub, sub)

    def as_2d(self) -> np.ndarray:
        return self.data.reshape(self.height, self.width)


@dataclass
class RGB:                      # Image.zig:132-170
    width: int
    height: int
    data: np.ndarray            # (height*width, 3) u8

    def getWidth(self) -> int:
        return self.width

    def getHeight(self) -> int:
        return self.height

    def getRGBLinear(self, index: int):
        return tuple(int(v) for v in self.data[index])

    def as_3d(self) -> np.ndarray:
        return self.data.reshape(self.height, self.width, 3)


@dataclass
class RGBA:                     # an RGBA text plan's image (fr_text_plan_create_rgba): the framebuffer's bytes
    width: int
    height: int
    data: np.ndarray            # (height*width, 4) u8, R G B A, not premultiplied (premultiplied from an over=True render)

    @staticmethod
    def init(width: int, height: int) -> "RGBA":
        return RGBA(width, height, np.zeros((width * height, 4), np.uint8))

    def unpremultiply(self, srgb: bool = False, *, device: bool = False, ctx=None) -> "RGBA":
        """fr_rgba_unpremultiply, in place: the premultiplied image of an over=True render (FR_TEXT_OVER) as straight
        alpha, which the RGBA QOI writer and image files expect.  srgb: the image was rendered with srgb=True, so the
        division is in linear light.  A pixel of alpha 0 becomes (0, 0, 0, 0); one of alpha 255 is unchanged.  Returns self.
        device: the same bytes through fr_layer_unpremultiply on the GPU (the image is uploaded and copied back)."""
        buf = rgba_pixels(self, "RGBA.unpremultiply", sized=device)
        if device:
            ctx = ctx or default_context()
            self.data[:] = round_trip(ctx, lambda p: layer_unpremultiply(ctx, p, self.width, self.width, self.height, srgb), buf)
            return self
        L.check(L.load_library().fr_rgba_unpremultiply(L.ptr(buf), buf.shape[0], 1 if srgb else 0))
        if buf is not self.data:
            self.data[:] = buf
        return self

    def over(self, layer: "RGBA", x: int = 0, y: int = 0, opacity: int = 255, srgb: bool = False, ctx=None) -> "RGBA":
        """fr_layer_over, in place: the premultiplied `layer` (an over=True render over a transparent background)
        composited over this premultiplied image with its top-left pixel at (x, y), whole pixels, clipped at the image's
        edges, at `opacity` in 0 .. 255.  srgb: both images are premultiplied in linear light (rendered with srgb=True).
        Both images are uploaded, composited on the device and this one copied back, as draw_text_rgba does.  Returns self."""
        dst, src = rgba_pixels(self, "RGBA.over: image"), rgba_pixels(layer, "RGBA.over: layer")
        if not 0 <= int(opacity) <= 255:
            raise ValueError(f"opacity {opacity!r}: expected 0 .. 255")
        if self.width == 0 or self.height == 0 or layer.width == 0 or layer.height == 0:
            return self
        ctx = ctx or default_context()
        blits = make_blits([(0, 0, layer.width, layer.height, int(x), int(y), int(opacity))])
        self.data[:] = round_trip(ctx, lambda d, s: layer_over(ctx, s, layer.width, layer.height, d, self.width, self.height,
                                                               blits, srgb), dst, src)
        return self

    def blend(self, layer: "RGBA", mode: int, x: int = 0, y: int = 0, opacity: int = 255, srgb: bool = False, ctx=None) -> "RGBA":
        """fr_layer_blend, in place: the premultiplied `layer` blended into this premultiplied image in `mode` (FR_BLEND_MULTIPLY,
        _SCREEN, _OVERLAY, _DARKEN, _LIGHTEN, _HARD_LIGHT, _DIFFERENCE, _EXCLUSION or _PLUS) with its top-left pixel at
        (x, y), whole pixels, clipped at the image's edges, at `opacity` in 0 .. 255.  srgb: both images are premultiplied in
        linear light.  Both images are uploaded, blended on the device and this one copied back, as over does.  Returns self."""
        dst, src = rgba_pixels(self, "RGBA.blend: image"), rgba_pixels(layer, "RGBA.blend: layer")
        if not 0 <= int(opacity) <= 255:
            raise ValueError(f"opacity {opacity!r}: expected 0 .. 255")
        if not 0 <= int(mode) < L.FR_BLEND_MODES:
            raise ValueError(f"mode {mode!r}: expected 0 .. {L.FR_BLEND_MODES - 1}")
        if self.width == 0 or self.height == 0 or layer.width == 0 or layer.height == 0:
            return self
        ctx = ctx or default_context()
        blits = make_blits([(0, 0, layer.width, layer.height, int(x), int(y), int(opacity))])
        self.data[:] = round_trip(ctx, lambda d, s: layer_blend(ctx, s, layer.width, layer.height, d, self.width, self.height,
                                                                blits, int(mode), srgb), dst, src)
        return self

    def over_warped(self, layer: "RGBA", matrix, opacity: int = 255, srgb: bool = False, ctx=None) -> "RGBA":
        """fr_layer_warp, in place: the premultiplied `layer` composited over this premultiplied image through the forward
        map `matrix` = ((a, b, tx), (c, d, ty)), layer pixels to image pixels with pixel centres at + 1/2: scaled, turned or
        moved by a fraction of a pixel, sampled bilinearly (warp_from_matrix makes the blit), clipped at the image's edges,
        at `opacity` in 0 .. 255.  Outside the layer the sample blends with transparent.  srgb: both images are premultiplied
        in linear light.  Both images are uploaded and this one copied back.  Returns self."""
        dst, src = rgba_pixels(self, "RGBA.over_warped: image"), rgba_pixels(layer, "RGBA.over_warped: layer")
        if not 0 <= int(opacity) <= 255:
            raise ValueError(f"opacity {opacity!r}: expected 0 .. 255")
        if self.width == 0 or self.height == 0 or layer.width == 0 or layer.height == 0:
            return self
        ctx = ctx or default_context()
        blits = make_warp_blits([warp_from_matrix(matrix, (0, 0, layer.width, layer.height), opacity)])
        self.data[:] = round_trip(ctx, lambda d, s: layer_warp(ctx, s, layer.width, layer.height, d, self.width, self.height,
                                                               blits, srgb), dst, src)
        return self

    def _masked(self, what: str, layer, mask, x, y, mask_xy, opacity, invert, srgb, ctx) -> "RGBA":
        """over_masked (layer an RGBA) and erase (layer None): one blit of fr_layer_mask over the part of the rectangle that
        the mask covers"""
        dst = rgba_pixels(self, f"{what}: image")
        src = None if layer is None else rgba_pixels(layer, f"{what}: layer")
        plane = isinstance(mask, Gray)
        if plane:
            m = mask.data
            if not isinstance(m, np.ndarray) or m.dtype != np.uint8 or m.shape != (mask.width * mask.height,):
                raise ValueError(f"{what}: mask.data must be a ({mask.width * mask.height},) uint8 array")
            m = np.ascontiguousarray(m)
        else:
            m = rgba_pixels(mask, f"{what}: mask")
        mx, my = int(mask_xy[0]), int(mask_xy[1])
        if not 0 <= int(opacity) <= 255:
            raise ValueError(f"opacity {opacity!r}: expected 0 .. 255")
        if mx < 0 or my < 0:
            raise ValueError(f"mask_xy {mask_xy!r}: expected an element of the mask")
        w, h = mask.width - mx, mask.height - my
        if layer is not None:
            w, h = min(w, layer.width), min(h, layer.height)
        if self.width == 0 or self.height == 0 or w <= 0 or h <= 0:
            return self
        ctx = ctx or default_context()
        blits = make_mask_blits([(0, 0, w, h, int(x), int(y), mx, my, int(opacity), 1 if invert else 0)])
        if layer is None:
            self.data[:] = round_trip(ctx, lambda d, k: layer_mask(ctx, None, 0, 0, k, mask.width, mask.height, d, self.width, self.height, blits,
                                                                   srgb, plane, True), dst, m)
        else:
            self.data[:] = round_trip(ctx, lambda d, s, k: layer_mask(ctx, s, layer.width, layer.height, k, mask.width, mask.height, d, self.width,
                                                                      self.height, blits, srgb, plane), dst, src, m)
        return self

    def over_masked(self, layer: "RGBA", mask, x: int = 0, y: int = 0, mask_xy=(0, 0), opacity: int = 255, invert: bool = False,
                    srgb: bool = False, ctx=None) -> "RGBA":
        """fr_layer_mask, in place: over() with an opacity per pixel.  The premultiplied `layer` lands with its top-left pixel
        at (x, y) and element mask_xy of `mask` lies over that pixel; each pixel is composited at m(k, opacity), where k is
        the mask's value there: the alpha of an RGBA mask (a layer: a panel, a shadow, an outline), or the byte of a Gray
        one (a coverage render).  invert: through 255 - k instead.  Only the part of the layer that the mask covers is
        drawn.  srgb: the images are premultiplied in linear light.  The three images are uploaded and this one copied back.
        Returns self."""
        return self._masked("RGBA.over_masked", layer, mask, x, y, mask_xy, opacity, invert, srgb, ctx)

    def erase(self, mask, x: int = 0, y: int = 0, mask_xy=(0, 0), opacity: int = 255, invert: bool = False, srgb: bool = False,
              ctx=None) -> "RGBA":
        """fr_layer_mask with FR_MASK_ERASE, in place: this premultiplied image is multiplied by 255 - m(k, opacity) where
        `mask` (an RGBA: its alpha; a Gray: its bytes) lies over it, element mask_xy on pixel (x, y) and the rest of the
        mask to its right and below: a knock-out, or underlines that skip the ink of a grown text layer.  invert: erase
        through 255 - k.  srgb: the image is premultiplied in linear light.  Returns self."""
        return self._masked("RGBA.erase", None, mask, x, y, mask_xy, opacity, invert, srgb, ctx)

    def fill_rects(self, rects, srgb: bool = False, ctx=None) -> "RGBA":
        """fr_layer_rects, in place: rects of (x0, y0, x1, y1, (R, G, B, A)) in float pixels, y down, each edge kept to 1/64
        pixel as floor(64 v + 1/2), filled with anti-aliased edges in their straight colours, in order, over this
        premultiplied image.  srgb: the image is premultiplied in linear light.  The image is uploaded, drawn into on the
        device and copied back.  Returns self."""
        dst = rgba_pixels(self, "RGBA.fill_rects")
        rows = []
        for x0, y0, x1, y1, colour in rects:
            edges = [q64(v) for v in (x0, y0, x1, y1)]
            if not all(-2 ** 31 <= e < 2 ** 31 for e in edges):
                raise ValueError(f"rectangle {(x0, y0, x1, y1)!r}: an edge beyond int32 in 1/64 pixel")
            rows.append((*edges, colour_rgba(colour, alpha_optional=False)))
        if not rows or self.width == 0 or self.height == 0:
            return self
        ctx = ctx or default_context()
        table = make_rects(rows)
        self.data[:] = round_trip(ctx, lambda d: layer_rects(ctx, d, self.width, self.height, table, srgb), dst)
        return self

    def paint(self, gradient, mask: "RGBA" = None, x: int = 0, y: int = 0, srgb: bool = False, ctx=None) -> "RGBA":
        """fr_layer_paint, in place: `gradient` (make_gradient_linear / make_gradient_radial, its geometry in 1/64 pixel of
        this image) composited over this premultiplied image through the alpha of the layer `mask` with its top-left pixel
        at (x, y), whole pixels, clipped at the image's edges: gradient text when the mask is an over=True render, a gradient
        glow when it is a shadow.  mask None: full coverage over the whole image, a gradient panel (x and y are not used).
        srgb: the image is premultiplied in linear light.  The images are uploaded, painted on the device and this one
        copied back.  Returns self."""
        dst = rgba_pixels(self, "RGBA.paint: image")
        if self.width == 0 or self.height == 0:
            return self
        ctx = ctx or default_context()
        if mask is None:
            self.data[:] = round_trip(ctx, lambda d: layer_paint(ctx, None, 0, 0, d, self.width, self.height, gradient,
                                                                 (0, 0, self.width, self.height), (0, 0), srgb), dst)
            return self
        src = rgba_pixels(mask, "RGBA.paint: mask")
        if mask.width == 0 or mask.height == 0:
            return self
        self.data[:] = round_trip(ctx, lambda d, s: layer_paint(ctx, s, mask.width, mask.height, d, self.width, self.height, gradient,
                                                                (0, 0, mask.width, mask.height), (int(x), int(y)), srgb), dst, src)
        return self

    def draw_lcd(self, plane: "Gray", x: int = 0, y: int = 0, rgba=(0, 0, 0, 255), weights=None, srgb: bool = False,
                 bgr: bool = False, ctx=None) -> "RGBA":
        """fr_layer_lcd, in place: sub-pixel (LCD) text.  `plane` is a coverage image three times as wide as the text it
        holds (element 3 u + j: sub-pixel j of pixel u; text.lcd_line renders one); it is filtered across sub-pixels with
        `weights` (FR_LCD_TAPS values that add up to 256; None: the default filter) and composited in the straight colour
        `rgba` over this premultiplied image with its pixel (0, 0) at (x, y), whole pixels, clipped at the image's edges,
        with an alpha of its own for each colour byte.  A plane width that is no multiple of 3 loses its last one or two
        elements.  srgb: the image is premultiplied in linear light; bgr: the panel's stripes are B G R.  Both images are
        uploaded and this one copied back.  Returns self."""
        dst = rgba_pixels(self, "RGBA.draw_lcd: image")
        cov = plane.data
        if not isinstance(cov, np.ndarray) or cov.dtype != np.uint8 or cov.shape != (plane.width * plane.height,):
            raise ValueError(f"RGBA.draw_lcd: plane.data must be a ({plane.width * plane.height},) uint8 array")
        colour = colour_rgba(rgba, alpha_optional=False)
        if self.width == 0 or self.height == 0 or plane.width < 3 or plane.height == 0:
            return self
        ctx = ctx or default_context()
        blits = make_lcd_blits([(0, 0, plane.width // 3, plane.height, int(x), int(y), colour)])
        self.data[:] = round_trip(ctx, lambda d, c: layer_lcd(ctx, c, plane.width, plane.height, d, self.width, self.height, blits,
                                                              weights, srgb, bgr), dst, np.ascontiguousarray(cov))
        return self

    def shadow(self, offset=(0, 0), spread: int = 0, blur_radius: int = 0, blur_passes: int = 0, rgba=(0, 0, 0, 255),
               pad: int = None, srgb: bool = False, ctx=None) -> "RGBA":
        """fr_layer_shadow of this premultiplied layer as a new premultiplied layer, `pad` pixels larger on every side
        (default: the reach spread + blur_passes * blur_radius, which holds the whole shadow at offset (0, 0)); pixel
        (pad, pad) of the result lies under pixel (0, 0) of this layer moved by `offset`.  Composite it with over(...,
        x - pad, y - pad), then this layer at (x, y).  The layer is uploaded and the shadow copied back."""
        src = rgba_pixels(self, "RGBA.shadow").reshape(-1)
        reach = int(spread) + (int(blur_passes) * int(blur_radius) if blur_radius and blur_passes else 0)
        pad = reach if pad is None else int(pad)
        if pad < 0:
            raise ValueError(f"pad {pad!r}: expected at least 0")
        out = RGBA.init(self.width + 2 * pad, self.height + 2 * pad)
        if out.width == 0 or out.height == 0:
            return out
        ctx = ctx or default_context()
        if src.size == 0:
            src = np.zeros(4, np.uint8)                     # an empty layer still needs an address
        out.data[:] = round_trip(ctx, lambda s, d: layer_shadow(
            ctx, s, self.width, self.height, d, out.width, out.height, (0, 0, self.width, self.height), (0, 0, out.width, out.height),
            (int(offset[0]) + pad, int(offset[1]) + pad), spread, blur_radius, blur_passes, rgba, srgb), src, out.data.shape, back=1)
        return out

    def outline(self, radius: int, kind: int = L.FR_OUTLINE_GROW, rgba=(0, 0, 0, 255), offset=(0, 0), pad: int = None,
                srgb: bool = False, ctx=None) -> "RGBA":
        """fr_layer_outline of this premultiplied layer as a new premultiplied layer, `pad` pixels larger on every side
        (default: the reach ceil(radius / 16), which holds the whole outline at offset (0, 0)); radius is in sixteenths of a
        pixel and kind one of FR_OUTLINE_GROW / _RING / _INNER / _SHRINK.  Pixel (pad, pad) of the result lies under pixel
        (0, 0) of this layer moved by `offset`: composite a GROW outline with over(..., x - pad, y - pad), then this layer at
        (x, y); an INNER line goes over the layer.  The layer is uploaded and the outline copied back."""
        src = rgba_pixels(self, "RGBA.outline").reshape(-1)
        pad = (int(radius) + 15) // 16 if pad is None else int(pad)
        if pad < 0:
            raise ValueError(f"pad {pad!r}: expected at least 0")
        out = RGBA.init(self.width + 2 * pad, self.height + 2 * pad)
        if out.width == 0 or out.height == 0:
            return out
        ctx = ctx or default_context()
        if src.size == 0:
            src = np.zeros(4, np.uint8)                     # an empty layer still needs an address
        out.data[:] = round_trip(ctx, lambda s, d: layer_outline(
            ctx, s, self.width, self.height, d, out.width, out.height, (0, 0, self.width, self.height), (0, 0, out.width, out.height),
            (int(offset[0]) + pad, int(offset[1]) + pad), radius, kind, rgba, srgb), src, out.data.shape, back=1)
        return out

    def getWidth(self) -> int:
        return self.width

    def getHeight(self) -> int:
        return self.height

    def as_3d(self) -> np.ndarray:
        return self.data.reshape(self.height, self.width, 4)


@dataclass
class GlyphDebug:               # Image.zig:173-241
    """Image.GlyphDebug: the exact-integer winding lattice (1 px per font unit, 1-unit border) coloured by
    setWindingLinear with the glyph's points marked; `render` runs on the device through fr_glyph_debug_render."""
    rgb: RGB
    winding_scale: int
    overflow_color: int = 150
    on_curve_color: tuple = (255, 255, 0)
    off_curve_color: tuple = (0, 255, 255)

    @staticmethod
    def render(glyph, winding_scale: int, *, ctx=None) -> "GlyphDebug":       # Image.zig:220
        ctx = ctx or default_context()
        gs = GlyphSet([glyph])
        box = glyph.box.as_array()
        W, H = int(box[2]) - int(box[0]) + 3, int(box[3]) - int(box[1]) + 3
        out = np.zeros((H * W, 3), np.uint8)
        L.check(ctx._lib.fr_glyph_debug_render(ctx._h, L.ptr(gs.points_xy), L.ptr(gs.contour_start), len(gs.contour_start) - 1,
                                               L.ptr(box), winding_scale, L.ptr(out)))
        return GlyphDebug(RGB(W, H, out), winding_scale)

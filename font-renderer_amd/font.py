"""Font — host-side mirror of /root/reference/src/font/Font.zig on the C ABI's contour producer
(fr_font_*: TrueType glyf/loca walk restated in C++, font-renderer_amd/csrc/fr_font.cpp).
Same surface as the reference: Font.initTTF(file) (:31), font.information (:25-29),
font.getGlyph(char) -> (Glyph, advance_width) (:161-169), plus glyph-index access and a
whole-font GlyphSet for batch rendering."""
from __future__ import annotations

import ctypes as C
from typing import Iterable, List, Optional

import numpy as np

from . import _lib as L
from .device import Handle
from .glyph import Box, Contour, FontInformation, Glyph, GlyphSet

FR_FONT_ALLOW_HINTED = 1


class Font(Handle):
    def __init__(self, data: bytes, allow_hinted: bool = False):
        self._lib = L.load_library()
        buf = (C.c_ubyte * len(data)).from_buffer_copy(data)
        self._open(self._lib.fr_font_close, self._lib.fr_font_open, buf, len(data), FR_FONT_ALLOW_HINTED if allow_hinted else 0)
        upm, ng, y0 = C.c_uint16(), C.c_uint16(), C.c_int()
        L.check(self._lib.fr_font_info(self._h, C.byref(upm), C.byref(ng), C.byref(y0)))
        self.information = FontInformation(upm.value, bool(y0.value))
        self.num_glyphs = ng.value

    @staticmethod
    def initTTF(path: str, allow_hinted: bool = False) -> "Font":       # Font.zig:31
        with open(path, "rb") as f:
            return Font(f.read(), allow_hinted)

    def glyph_index(self, char: int) -> int:                           # CharGlyphMapping.getGlyph
        gi = C.c_uint16()
        L.check(self._lib.fr_font_char_to_glyph(self._h, char, C.byref(gi)))
        return gi.value

    def glyph_by_index(self, gi: int) -> Glyph:                        # Font.zig:171 loadGlyph
        nc, npnt = C.c_uint32(), C.c_uint32()
        box = np.zeros(4, np.int16)
        L.check(self._lib.fr_font_glyph_measure(self._h, gi, C.byref(nc), C.byref(npnt), L.ptr(box)))
        pts = np.zeros((max(npnt.value, 1), 2), np.int16)
        cs = np.zeros(nc.value + 1, np.uint32)
        L.check(self._lib.fr_font_glyph_fill(self._h, gi, L.ptr(pts), L.ptr(cs)))
        contours = [Contour(pts[int(cs[c]):int(cs[c + 1])].copy()) for c in range(nc.value)]
        return Glyph(Box(int(box[0]), int(box[1]), int(box[2]), int(box[3])), contours)

    def advance_width(self, gi: int) -> int:                           # Font.advance_widths[gi] (Font.zig:123-139)
        a = C.c_int16()
        L.check(self._lib.fr_font_glyph_advance(self._h, gi, C.byref(a)))
        return a.value

    def layout(self, text, font_size: int):
        """fr_text_layout: the reference's pen walk (Appli.zig:318-349) over `text` (a str or code points) ->
        (glyph indices u16, pen_x64 i32 — 1/64 pixel, half up —, end pen_x64).  No kerning, no line breaking."""
        cps = np.array([ord(c) for c in text] if isinstance(text, str) else list(text), np.uint32)
        gi = np.zeros(max(len(cps), 1), np.uint16)
        pen = np.zeros(max(len(cps), 1), np.int32)
        end = C.c_int32()
        L.check(self._lib.fr_text_layout(self._h, L.ptr(cps), len(cps), font_size, L.ptr(gi), L.ptr(pen), C.byref(end)))
        return gi[:len(cps)], pen[:len(cps)], end.value

    def line_metrics(self) -> dict:
        """fr_font_line_metrics: hhea's ascender, descender and line_gap, post's underline_position (the top of the line)
        and underline_thickness, OS/2's strikeout_size and strikeout_position, in font units, y up; `present`: bit 0 post,
        bit 1 OS/2 (an absent table's values are 0)"""
        m = L.FontLine()
        L.check(self._lib.fr_font_line_metrics(self._h, C.byref(m)))
        return {name: getattr(m, name) for name, _ in L.FontLine._fields_}

    def decoration(self, font_size: int, kind: int):
        """fr_text_decoration: (top, bottom) of the underline (FR_DECOR_UNDERLINE), the strike-out (FR_DECOR_STRIKEOUT) or
        the line box (FR_DECOR_LINE_BOX) at font_size, as offsets from the baseline in 1/64 pixel, y down"""
        top, bottom = C.c_int32(), C.c_int32()
        L.check(self._lib.fr_text_decoration(self._h, font_size, kind, C.byref(top), C.byref(bottom)))
        return top.value, bottom.value

    def getGlyph(self, char: int):                                   # Font.zig:161-169 -> struct {Glyph, i16}
        gi = self.glyph_index(char)
        return self.glyph_by_index(gi), self.advance_width(gi)

    def glyphset(self, glyph_indices: Optional[Iterable[int]] = None, skip_unsupported: bool = True):
        """-> (GlyphSet, kept glyph indices): the whole font (or the given indices) ready for
        fr_glyphset_create; glyphs the reference would panic on are skipped when asked."""
        idx = range(self.num_glyphs) if glyph_indices is None else glyph_indices
        glyphs: List[Glyph] = []
        kept: List[int] = []
        for gi in idx:
            try:
                glyphs.append(self.glyph_by_index(gi))
                kept.append(gi)
            except L.FrError:
                if not skip_unsupported:
                    raise
        return GlyphSet(glyphs), kept

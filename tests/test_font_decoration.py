"""fr_font_line_metrics and fr_text_decoration (include/fr_raster.h; host only): the metrics of the four committed fonts
against fontTools' hhea, post and OS/2, the decoration rows against the header's R in exact fractions, and fonts whose post or
OS/2 table is missing or cut short.  No GPU."""
import struct
from fractions import Fraction
from math import floor

import pytest
from fontTools.ttLib import TTFont

import font_renderer_amd as fr
from fixtures import font_bytes, font_file, load_font

FONTS = ("DejaVuSans.ttf", "DejaVuSansMono.ttf", "DejaVuSerif-Italic.ttf", "STIXGeneral.ttf")


def _want(name):
    tt = TTFont(font_file(name))
    return {"ascender": tt["hhea"].ascent, "descender": tt["hhea"].descent, "line_gap": tt["hhea"].lineGap,
            "underline_position": tt["post"].underlinePosition, "underline_thickness": tt["post"].underlineThickness,
            "strikeout_size": tt["OS/2"].yStrikeoutSize, "strikeout_position": tt["OS/2"].yStrikeoutPosition, "present": 3}


@pytest.mark.parametrize("name", FONTS)
def test_line_metrics_are_the_tables_values(name):
    font = load_font(name, allow_hinted=True)
    assert font.line_metrics() == _want(name)


def test_the_reference_values():
    m = load_font("DejaVuSans.ttf", allow_hinted=True).line_metrics()
    assert (m["ascender"], m["descender"], m["line_gap"]) == (1901, -483, 0)
    assert (m["underline_position"], m["underline_thickness"]) == (-130, 90) and (m["strikeout_size"], m["strikeout_position"]) == (102, 530)
    m = load_font("STIXGeneral.ttf", allow_hinted=True).line_metrics()
    assert (m["ascender"], m["descender"], m["line_gap"]) == (1055, -455, 0)
    assert (m["underline_position"], m["underline_thickness"]) == (-75, 50) and (m["strikeout_size"], m["strikeout_position"]) == (50, 306)


def _R(v, size, upm):
    return floor(Fraction(128 * size * v + upm, 2 * upm))


@pytest.mark.parametrize("size", [9, 32, 200])
@pytest.mark.parametrize("name", FONTS)
def test_decoration_rows_are_the_rounded_metrics(name, size):
    font = load_font(name, allow_hinted=True)
    m, upm = font.line_metrics(), font.information.units_per_em
    top = -_R(m["underline_position"], size, upm)
    assert font.decoration(size, fr.FR_DECOR_UNDERLINE) == (top, top + max(1, _R(m["underline_thickness"], size, upm)))
    top = -_R(m["strikeout_position"], size, upm)
    assert font.decoration(size, fr.FR_DECOR_STRIKEOUT) == (top, top + max(1, _R(m["strikeout_size"], size, upm)))
    assert font.decoration(size, fr.FR_DECOR_LINE_BOX) == (-_R(m["ascender"], size, upm), -_R(m["descender"], size, upm))
    # the underline lies below the baseline, the stroke above it, the box around both
    u, s, b = (font.decoration(size, k) for k in (fr.FR_DECOR_UNDERLINE, fr.FR_DECOR_STRIKEOUT, fr.FR_DECOR_LINE_BOX))
    assert b[0] < s[0] < s[1] <= 0 < u[0] < u[1] <= b[1]


def test_rounding_is_a_true_floor_for_negative_values():
    """R(-130) at size 9 and 2048 units per em is floor(-36.06..) = -37; a division that truncates would give -36"""
    assert _R(-130, 9, 2048) == floor(Fraction(-130 * 9 * 64, 2048) + Fraction(1, 2)) == -37
    assert load_font("DejaVuSans.ttf", allow_hinted=True).decoration(9, fr.FR_DECOR_UNDERLINE)[0] == 37


def _without(data: bytes, tag: bytes, new_length=None) -> bytes:
    """the font with the directory entry of `tag` renamed away (the table's bytes stay where they are), or with its
    length field set to new_length"""
    n = struct.unpack(">H", data[4:6])[0]
    for t in range(n):
        e = 12 + 16 * t
        if data[e:e + 4] == tag:
            if new_length is None:
                return data[:e] + b"zzzz" + data[e + 4:]
            return data[:e + 12] + struct.pack(">I", new_length) + data[e + 16:]
    raise AssertionError(f"no {tag!r} table")


def test_a_font_without_post_still_opens():
    data = font_bytes("DejaVuSans.ttf")
    font = fr.Font(_without(data, b"post"), True)
    m = font.line_metrics()
    assert m["present"] == 2 and (m["underline_position"], m["underline_thickness"]) == (0, 0)
    assert (m["ascender"], m["strikeout_size"], m["strikeout_position"]) == (1901, 102, 530)
    with pytest.raises(fr.FrError) as e:
        font.decoration(32, fr.FR_DECOR_UNDERLINE)
    assert e.value.code == -4
    assert font.decoration(32, fr.FR_DECOR_STRIKEOUT) == load_font("DejaVuSans.ttf", True).decoration(32, fr.FR_DECOR_STRIKEOUT)
    assert font.glyph_index(ord("A")) == load_font("DejaVuSans.ttf", True).glyph_index(ord("A"))


def test_missing_or_truncated_tables_clear_their_bits():
    data = font_bytes("DejaVuSans.ttf")
    font = fr.Font(_without(data, b"OS/2"), True)
    assert font.line_metrics()["present"] == 1
    with pytest.raises(fr.FrError) as e:
        font.decoration(32, fr.FR_DECOR_STRIKEOUT)
    assert e.value.code == -4
    assert font.decoration(32, fr.FR_DECOR_LINE_BOX)[0] < 0
    assert fr.Font(_without(data, b"post", 11), True).line_metrics()["present"] == 2          # the thickness would end at byte 12
    assert fr.Font(_without(data, b"post", 12), True).line_metrics()["present"] == 3
    assert fr.Font(_without(data, b"OS/2", 29), True).line_metrics()["present"] == 1          # the position would end at byte 30
    assert fr.Font(_without(_without(data, b"OS/2"), b"post"), True).line_metrics()["present"] == 0


def test_refusals():
    font = load_font("DejaVuSans.ttf", allow_hinted=True)
    with pytest.raises(fr.FrError) as e:
        font.decoration(32, 3)
    assert e.value.code == -1
    lib = fr.load_library()
    import ctypes as C
    top = C.c_int32()
    assert lib.fr_text_decoration(font._h, 32, 0, C.byref(top), None) == -1 and lib.fr_text_decoration(font._h, 32, 0, None, C.byref(top)) == -1
    assert lib.fr_text_decoration(None, 32, 0, C.byref(top), C.byref(top)) == -1 and lib.fr_font_line_metrics(font._h, None) == -1
    assert lib.fr_font_line_metrics(None, C.byref(fr.FontLine())) == -1

"""CPU suite for fr_text_layout, the reference's pen walk (Appli.zig:318-349): glyphs from cmap, pens from the
cumulative advances read independently with fontTools, rounded to 1/64 pixel half up in exact integers."""
import numpy as np
import pytest

import font_renderer_amd as fr
from fixtures import font_file, load_font

FONTS = ["DejaVuSans.ttf", "DejaVuSansMono.ttf", "DejaVuSerif-Italic.ttf", "STIXGeneral.ttf"]


def _tt(name):
    from fontTools.ttLib import TTFont
    return TTFont(font_file(name))


def _advance(tt, gname):
    """advance_widths[g] as the reference fills it (Font.zig:123-139): the LongHorMetric's advance read as i16 for the
    first numberOfHMetrics glyphs, the i16 entry after the long metrics (the left side bearing) for the others"""
    order = tt.getGlyphOrder()
    adv, lsb = tt["hmtx"][gname]
    if order.index(gname) < tt["hhea"].numberOfHMetrics:
        return int(np.int16(np.uint16(adv)))
    return int(lsb)


def _pens(tt, gnames, font_size):
    upm = tt["head"].unitsPerEm
    e, out = 0, []
    for g in gnames + [None]:
        out.append((128 * font_size * e + upm) // (2 * upm))          # floor: round half up of 64 * size * E / upm
        if g is not None:
            e += _advance(tt, g)
    return out[:-1], out[-1]


@pytest.mark.parametrize("name", FONTS)
@pytest.mark.parametrize("font_size", [7, 16, 32, 61])
def test_pens_match_fonttools(name, font_size):
    tt = _tt(name)
    cmap, order = tt.getBestCmap(), tt.getGlyphOrder()
    text = "Hello, World! ffi fj Tf AVAWAY 0123456789 {[(|)]} ~^`"
    font = load_font(name)
    gi, pen, end = font.layout(text, font_size)
    gnames = [cmap.get(ord(c), order[0]) for c in text]
    assert [order[g] for g in gi] == gnames
    want, want_end = _pens(tt, gnames, font_size)
    assert pen.tolist() == want
    assert end == want_end


def test_lsb_as_advance_past_the_long_metrics():
    """DejaVuSansMono has 4 long metrics: every printable glyph's advance is its lsb entry, some negative (IJ: -1)"""
    tt = _tt("DejaVuSansMono.ttf")
    assert tt["hhea"].numberOfHMetrics < 10
    font = load_font("DejaVuSansMono.ttf")
    text = "AĲĳŁB" * 3
    gi, pen, end = font.layout(text, 24)
    names = [tt.getBestCmap()[ord(c)] for c in text]
    adv = [_advance(tt, g) for g in names]
    assert min(adv) < 0 and all(a != tt["hmtx"][g][0] for a, g in zip(adv, names) if a < 0)
    assert [font.advance_width(int(g)) for g in gi] == adv
    want, want_end = _pens(tt, names, 24)
    assert pen.tolist() == want and end == want_end


def test_unmapped_code_points_give_glyph_zero():
    font = load_font("DejaVuSerif-Italic.ttf")
    gi, pen, _ = font.layout([0x10FFFD, ord("a"), 0xE000, 0x1F600], 20)
    assert gi[0] == 0 and gi[2] == 0 and gi[3] == 0 and gi[1] != 0
    assert pen[0] == 0
    assert pen[1] == (128 * 20 * font.advance_width(0) + 2048) // 4096


def test_negative_and_large_sums_round_as_specified():
    tt = _tt("DejaVuSansMono.ttf")
    font = load_font("DejaVuSansMono.ttf")
    # a negative running sum: only negative advances (IJ, ij, Lslash), every size, including exact halves
    text = "ĲĳŁ" * 40
    names = [tt.getBestCmap()[ord(c)] for c in text]
    for size in (1, 3, 16, 100, 1000, 65535):
        gi, pen, end = font.layout(text, size)
        want, want_end = _pens(tt, names, size)
        assert end < 0 and pen.tolist() == want and end == want_end, size
    # large sums: 20 000 'W' of DejaVuSans at size 1000 -> the last pens above 2^30 (1/64 pixel), still exact
    tt = _tt("DejaVuSans.ttf")
    font = load_font("DejaVuSans.ttf")
    text = "W" * 20000
    gi, pen, end = font.layout(text, 1000)
    want, want_end = _pens(tt, [tt.getBestCmap()[ord("W")]] * len(text), 1000)
    assert pen.tolist() == want and end == want_end and end > 2 ** 30
    # ties: E * 64 * size / upm exactly halfway between two 1/64 steps rounds up
    ties = [k for k, p in enumerate(want) if ((128 * 1000 * (k * _advance(tt, "W"))) % 4096) == 2048]
    assert ties and all(int(pen[k]) * 4096 - 128 * 1000 * k * _advance(tt, "W") == 2048 for k in ties[:50])
    # a pen beyond int32 is an error, not a wrapped value
    with pytest.raises(fr.FrError) as e:
        font.layout(text, 2000)
    assert e.value.code == -1

"""CPU suite for the twin of fr_glyph_place_affine text plans (tests/text_twin.py) and for the Python layout that
feeds them (font_renderer_amd/text.py), no GPU: (a) the upright, power-of-two case is fr_glyph_place_ex bit for bit;
(b) on block glyphs under exact maps the twin equals the winding decided with Fractions; (c) the cell holds the glyph;
(d) rotated_line's pens and matrices."""
import math
from fractions import Fraction as Fr

import numpy as np
import pytest

import text_affine_cases as ac
import text_block_cases as bc
import text_twin as tw
from fixtures import load_font
from font_renderer_amd import render_glyph as rg
from font_renderer_amd import text as T

STRINGS = ["ffi fj Tf", "Wavy /// fff"]
GRIDS = [(4, True), (4, False), (2, True), (2, False), (1, True), (1, False)]


def _ex_lines(font_name, font_size, s, k, seed):
    """the strings as fr_glyph_place_ex runs at scale s and slant k, every pen with its own fractions in both axes"""
    font = load_font(font_name, allow_hinted=True)
    gs, places, runs, _ = tw.lines(font, STRINGS, font_size, pad=3)
    rng = np.random.default_rng(seed)
    ex = rg.make_places_ex([(int(p["glyph"]), int(p["pen_x64"]), 64 * int(p["pen_y"]) + int(rng.integers(0, 64)), s, k) for p in places])
    return gs, ex, runs


# ---- (a) consequence 1: m = {s, s k, 0, s}, s a power of two, is fr_glyph_place_ex bit for bit ---------------------------
@pytest.mark.parametrize("s,font_size", [(1 / 64, 32), (1 / 32, 64), (1 / 16, 128)])
@pytest.mark.parametrize("k", [0.0, 0.2, -1.0])
def test_upright_power_of_two_equals_the_ex_twin(s, font_size, k):
    n, center = ((4, True), (2, False), (1, True))[int(round(math.log2(s * 64)))]
    gs, ex, runs = _ex_lines("DejaVuSerif-Italic.ttf" if k else "DejaVuSans.ttf", font_size, s, k, font_size)
    af = tw.from_ex(ex, runs)
    assert af["m"][0, 1] == np.float32(s) * np.float32(k) and af["m"][0, 2] == 0
    rng = np.random.default_rng(3)
    colours = rng.integers(0, 256, (len(ex), 4)).astype(np.uint8)
    clear = rng.integers(0, 256, 4).astype(np.uint8)
    for r in range(len(runs)):
        for idx in range(int(runs[r]["first"]), int(runs[r]["first"]) + int(runs[r]["count"])):
            g, px, py, ps, pk = tw.ex_place_params(ex[idx], runs[r])
            assert tw.affine_cell(gs.boxes[g], af[idx]["m"], px, py) == tw.ex_cell(gs.boxes[g], ps, pk, px, py), idx
        for fill in (False, True):
            want = tw.coverage_samples("ex", gs, ex, runs[r], n, center, fill)
            assert want.any()
            assert np.array_equal(tw.coverage_samples("affine", gs, af, runs[r], n, center, fill), want), (r, fill)
            assert np.array_equal(tw.rgba_samples("affine", gs, af, colours, runs[r], clear, None, n, center, fill),
                                  tw.rgba_samples("ex", gs, ex, colours, runs[r], clear, None, n, center, fill)), (r, fill)
    assert np.array_equal(tw.rgba_render_run("affine", gs, af, colours, runs[1], clear, None, n, center, True, srgb=True, bgr=True),
                          tw.rgba_render_run("ex", gs, ex, colours, runs[1], clear, None, n, center, True, srgb=True, bgr=True))


def test_inverse_is_binary64_as_defined():
    """two rounded products, one rounded difference, four rounded quotients rounded once more to binary32"""
    m = np.array([0.0137, -0.0071, 0.0069, 0.0141], np.float32)
    xx, xy, yx, yy = (float(v) for v in m)
    det = xx * yy - xy * yx                                # (Python floats: binary64, one rounding per operation)
    want = tuple(np.float32(v) for v in (yy / det, -xy / det, -yx / det, xx / det))
    assert tw.inverse(m) == want
    assert tw.inverse((0.5, 0.0, 0.0, 0.5)) == (2.0, 0.0, 0.0, 2.0)
    assert tw.inverse((0.0, -0.25, 0.25, 0.0)) == (0.0, 4.0, -4.0, 0.0)      # a quarter turn: consequence 3


# ---- (b) block glyphs under the eight exact maps: the twin against Fractions ------------------------------------------------
@pytest.mark.parametrize("n,center", GRIDS)
def test_twin_equals_the_exact_winding_on_block_glyphs(n, center):
    glyphs, places, runs, _ = ac.block_case(n, center)
    gs = bc.glyph_set(glyphs)
    assert {tuple(Fr(float(v)) / s for v in p["m"]) for p in places for s in ac.SCALES} >= set(ac.MAPS)
    assert {(int(p["pen_x64"]) % 64, int(p["pen_y64"]) % 64) for p in places} == {(0, 0), (37, 0), (0, 37), (37, 37)}
    for run in runs:
        exact = ac.instance_hits(glyphs, places, run, n, center)          # (asserts the margin condition, sample by sample)
        twin = tw.instance_hits("affine", gs, places, run, n, center, fill=True)
        assert [e[:3] for e in exact] == [t[:3] for t in twin]
        for (idx, y0, x0, hit, cx, cy), (_, _, _, thit) in zip(exact, twin):
            g, px, py, m = tw.affine_place_params(places[idx])
            fcx, fcy = tw.affine_sample_coords(m, px, py, x0, x0 + len(cx[0]) // n, y0, y0 + len(cx) // n, n, center)
            assert np.array_equal(fcx.astype(np.float64), np.array(cx, np.float64)), idx   # every (cx, cy) is the exact value
            assert np.array_equal(fcy.astype(np.float64), np.array(cy, np.float64)), idx
            assert np.array_equal(thit, hit), (idx, n, center)
            assert hit.any() and not hit.all()


def test_block_case_reaches_tile_borders_and_clips_on_four_sides():
    glyphs, places, runs, shape = ac.block_case(4, True)
    met = tw.met_tiles("affine", bc.glyph_set(glyphs), places, runs)
    assert {(2, 0, 0), (2, 0, 1), (2, 1, 0), (2, 1, 1)} <= met and len({t for t in met if t[0] == 0}) >= 20
    cells = [ac.cell(glyphs[int(p["glyph"])].box, ac.place_of(p)[3], int(p["pen_x64"]), int(p["pen_y64"])) for p in places[:24]]
    assert any(c0 < 64 < c0 + cw or c0 < 128 < c0 + cw for c0, _, cw, _ in cells)          # a cell across a 64-column border
    assert sum(1 for _, r0, _, ch in cells if r0 // 16 != (r0 + ch - 1) // 16) >= 12       # and across 16-row borders
    k = int(runs[1]["first"])
    c0, r0, cw, ch = ac.cell(glyphs[int(places[k]["glyph"])].box, ac.place_of(places[k])[3], int(places[k]["pen_x64"]), int(places[k]["pen_y64"]))
    assert c0 < 0 and r0 < 0 and c0 + cw > int(runs[1]["w"]) and r0 + ch > int(runs[1]["h"])
    curved = [g for g in GRIDS if any(int(p["glyph"]) == 8 for p in ac.block_case(*g)[1])]
    assert len(curved) >= 3, curved                                    # the curved outline takes part on these grids
    for r in runs:
        assert int(r["out_y"]) + int(r["h"]) < shape[0] and int(r["out_x"]) + int(r["w"]) < shape[1]


# ---- (c) the cell holds the glyph ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,center", [(4, True), (2, False), (1, False)])
def test_widening_the_cell_changes_nothing_on_block_glyphs(n, center):
    glyphs, places, runs, _ = ac.block_case(n, center)
    for run in runs[:1]:
        for idx, _, _, hit, _, _ in ac.instance_hits(glyphs, places, run, n, center, widen=1):
            ring = hit.copy()
            ring[n:-n, n:-n] = False
            assert not ring.any(), idx


def _rotated(font_name, size, angle, slant=0.0, mirror=False):
    font = load_font(font_name, allow_hinted=True)
    c, s = math.cos(math.radians(angle)), math.sin(math.radians(angle))
    gs, places, runs = T.rotated_line(font, "Tfy jg/", size, angle, 80.3 - 45 * c, 48.6 + 30 * s, 160, 96, slant=slant)
    if mirror:
        places["m"][:, 0] *= -1
        places["m"][:, 2] *= -1
    return gs, places, runs


@pytest.mark.parametrize("angle,font_name,size", [(7, "DejaVuSans.ttf", 14), (33, "DejaVuSerif-Italic.ttf", 29), (90, "DejaVuSans.ttf", 29),
                                                  (-120, "DejaVuSerif-Italic.ttf", 14), (0, "DejaVuSans.ttf", 29)])
def test_widening_the_cell_changes_nothing_on_rotated_lines(angle, font_name, size):
    gs, places, runs = _rotated(font_name, size, angle, slant=0.2 if angle == 33 else 0.0)
    n = 2
    inner = tw.instance_hits("affine", gs, places, runs[0], n, True, fill=True)
    for idx in range(len(places)):
        if not gs.segments_per_glyph()[int(places[idx]["glyph"])]:
            continue
        one = np.array(runs[0]).copy()
        one["first"], one["count"], one["w"], one["h"] = idx, 1, 65535, 65535
        pl = places.copy()
        pl["pen_x64"] += 64 * 300                                       # far from every edge of a huge run: nothing is clipped
        pl["pen_y64"] += 64 * 300
        (_, y0, x0, hit), = tw.instance_hits("affine", gs, pl, one, n, True, fill=True, widen=1)
        ring = hit.copy()
        ring[n:-n, n:-n] = False
        assert not ring.any() and hit.any(), idx
    assert len(inner) >= 5


# ---- (d) rotated_line -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("angle,zoom,slant", [(7.0, 1.0, 0.0), (33.0, 1.25, 0.2), (90.0, 1.0, 0.0), (-120.0, 0.75, -0.36), (180.0, 2.0, 0.0),
                                              (270.0, 1.0, 0.2)])
def test_rotated_line_follows_its_formula(angle, zoom, slant):
    font = load_font("DejaVuSans.ttf", allow_hinted=True)
    text, size, x, y = "Axis title", 16, 40.3, 71.77
    gi, pen, _ = font.layout(text, size)
    gs, places, runs = T.rotated_line(font, text, size, angle, x, y, 160, 96, zoom, slant)
    exact = {90.0: (0.0, 1.0), 180.0: (-1.0, 0.0), 270.0: (0.0, -1.0)}
    c, sn = exact.get(angle, (math.cos(math.radians(angle)), math.sin(math.radians(angle))))
    s = size * zoom / font.information.units_per_em
    m = np.array([s * c, s * (c * slant - sn), s * sn, s * (sn * slant + c)]).astype(np.float32)
    assert len(places) == len(gi) and places.dtype == rg.PLACE_AFFINE_DTYPE
    for k, p in enumerate(places):
        assert int(p["pen_x64"]) == math.floor(64.0 * (x + c * zoom * int(pen[k]) / 64.0) + 0.5)
        assert int(p["pen_y64"]) == math.floor(64.0 * (y - sn * zoom * int(pen[k]) / 64.0) + 0.5)
        assert np.array_equal(p["m"], m)
    assert (int(runs[0]["w"]), int(runs[0]["h"]), int(runs[0]["count"])) == (160, 96, len(places))
    if angle == 90.0 and slant == 0.0:
        assert tuple(places[0]["m"]) == (0.0, -np.float32(s), np.float32(s), 0.0)           # consequence 3


@pytest.mark.parametrize("slant", [0.0, 0.2])
def test_rotated_line_at_zero_degrees_is_view_line(slant):
    font = load_font("DejaVuSans.ttf", allow_hinted=True)
    upm = font.information.units_per_em
    size, zoom = 16, upm / 1024.0                                         # scale 1/64, a power of two
    assert np.float32(size * zoom / upm) == np.float32(1 / 64) and (size * zoom / upm) == 1 / 64
    view = T.view_line(font, "Tfy jg/", size, zoom, 10.25, 40.5, 160, 96, slant)
    rot = T.rotated_line(font, "Tfy jg/", size, 0.0, 10.25, 40.5, 160, 96, zoom, slant)
    assert view is not None and rot is not None
    (_, vp, vr), (_, rp, rr) = view, rot
    assert np.array_equal(vp["glyph"], rp["glyph"]) and np.array_equal(vp["pen_x64"], rp["pen_x64"])
    assert np.array_equal(vp["pen_y64"], rp["pen_y64"])
    assert np.array_equal(tw.from_ex(vp, vr)["m"], rp["m"])
    assert T.rotated_line(font, "", size, 0.0, 0, 0, 10, 10) is None and T.rotated_line(font, "a", size, 0.0, 0, 0, 0, 10) is None
    with pytest.raises(ValueError):
        T.rotated_line(font, "a", size, float("nan"), 0, 0, 10, 10)
    box = font.glyphset([int(font.layout("T", size)[0][0])], skip_unsupported=False)[0].boxes[0]
    assert T.instance_cell_affine(box, rp["m"][0], 37, 64 * 9 + 5) == tw.affine_cell(box, rp["m"][0], 37, 64 * 9 + 5)
    assert T.instance_cell_affine(box, (1 / 64, 0.0, 0.0, 1 / 64), 37, 64 * 9 + 5) == T.instance_cell_ex(box, 1 / 64, 0.0, 37, 64 * 9 + 5)

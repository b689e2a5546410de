"""CPU suite for the twin of fr_glyph_place_ex text plans (tests/text_twin.py) and for the Python layout that feeds
them (font_renderer_amd/text.py), no GPU: the two consequences of the definition (include/fr_raster.h) — degenerate
parameters are fr_glyph_place bit for bit, a +64 shift of pen_y64 is a one-row shift —, that the slanted cell holds the
glyph, the span layout, and the validation of the new Python arguments."""
import numpy as np
import pytest

import text_twin as tw
from fixtures import load_font
from font_renderer_amd import render_glyph as rg
from font_renderer_amd import text as T
from text_gpu import degenerate

STRINGS = ["ffi fj Tf ff", "Tjfyfgf jjj", "Wavy /// fff", "ƒ∫ fî T,"]
SLANTS = [-1.0, -0.36, -0.2, 0.0, 0.2, 0.36397, 1.0, 4.0]          # those of tests/test_gpu_text_place.py's twin test


def _random_instances(ascii_set, rng, count):
    """`count` single-instance runs over random glyphs of the committed ASCII set: sizes 12 .. 48, fractional pens"""
    gs = ascii_set.gs
    seg = gs.segments_per_glyph()
    rows, runs = [], []
    while len(rows) < count:
        g = int(rng.integers(len(ascii_set)))
        if not seg[g]:
            continue
        scale = np.float32(int(rng.integers(12, 49))) / np.float32(int(ascii_set.g_upm[g]))
        pen_x64 = int(rng.integers(0, 64))
        c0, r0, w, h = tw.plain_cell(gs.boxes[g], scale, pen_x64, 0)
        runs.append((len(rows), 1, w + 2, h + 2, 0, 0, scale))
        rows.append((g, pen_x64 - 64 * c0 + 64, -r0 + 1))
    return rg.make_places(rows), rg.make_runs(runs)


# ---- consequence 1: degenerate parameters are fr_glyph_place, bit for bit ----------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 4])
@pytest.mark.parametrize("center", [False, True])
@pytest.mark.parametrize("fill", [False, True])
def test_degenerate_equals_text_ref_on_the_ascii_set(ascii_set, n, center, fill):
    rng = np.random.default_rng(1000 + 10 * n + 2 * center + fill)
    places, runs = _random_instances(ascii_set, rng, 12)
    for r in range(len(runs)):
        want = tw.coverage_samples("plain", ascii_set.gs, places, runs[r], n, center, fill)
        for scale in (0.0, float(runs[r]["scale"])):
            got = tw.coverage_samples("ex", ascii_set.gs, degenerate(places, scale), runs[r], n, center, fill)
            assert np.array_equal(got, want), (r, n, center, fill, scale)
        k = int(runs[r]["first"])
        assert (tw.ex_cell(ascii_set.gs.boxes[int(places[k]["glyph"])], runs[r]["scale"], 0.0, int(places[k]["pen_x64"]), 64 * int(places[k]["pen_y"]))
                == tw.plain_cell(ascii_set.gs.boxes[int(places[k]["glyph"])], runs[r]["scale"], int(places[k]["pen_x64"]), int(places[k]["pen_y"])))


@pytest.mark.parametrize("font_size,n,center", [(16, 4, True), (23, 2, False), (40, 1, True), (11, 4, False)])
def test_degenerate_equals_the_twins_on_italic_strings(font_size, n, center):
    font = load_font("DejaVuSerif-Italic.ttf")
    gs, places, runs, _ = tw.lines(font, STRINGS, font_size, pad=2)
    ex = degenerate(places)
    rng = np.random.default_rng(font_size)
    colours = rng.integers(0, 256, (len(places), 4)).astype(np.uint8)
    clear = rng.integers(0, 256, 4).astype(np.uint8)
    for fill in (False, True):
        for r in range(len(runs)):
            assert np.array_equal(tw.coverage_samples("ex", gs, ex, runs[r], n, center, fill),
                                  tw.coverage_samples("plain", gs, places, runs[r], n, center, fill)), (r, fill)
            assert np.array_equal(tw.rgba_samples("ex", gs, ex, colours, runs[r], clear, None, n, center, fill),
                                  tw.rgba_samples("plain", gs, places, colours, runs[r], clear, None, n, center, fill)), (r, fill)
    r = 1
    assert np.array_equal(tw.rgba_render_run("ex", gs, ex, colours, runs[r], clear, None, n, center, False, srgb=True, bgr=True),
                          tw.rgba_render_run("plain", gs, places, colours, runs[r], clear, None, n, center, False, srgb=True, bgr=True))


# ---- consequence 2: pen_y64 + 64 is the same image one row down --------------------------------------------------------
@pytest.mark.parametrize("fill", [False, True])
def test_a_64_shift_of_pen_y64_is_one_row(ascii_set, fill):
    gs = ascii_set.gs
    rng = np.random.default_rng(64 + fill)
    g = ascii_set.find("Serif", "g")
    for fy64 in range(64):
        n, center = [(1, False), (2, True), (4, True), (4, False)][fy64 % 4]
        scale = np.float32(int(rng.integers(12, 49))) / np.float32(int(ascii_set.g_upm[g]))
        slant = float(rng.choice(SLANTS))
        pen_x64 = int(rng.integers(0, 64))
        c0, r0, w, h = tw.ex_cell(gs.boxes[g], scale, slant, pen_x64, fy64)
        run = rg.make_runs([(0, 1, w + 2, h + 3, 0, 0, np.float32(1.0))])[0]
        at = lambda y64: tw.coverage_samples("ex", gs, rg.make_places_ex([(g, pen_x64 - 64 * c0 + 64, y64, scale, slant)]), run, n, center, fill)
        base, down = at(fy64 - 64 * r0 + 64), at(fy64 - 64 * r0 + 128)
        assert base.any()
        assert np.array_equal(down[n:], base[:-n]) and not down[:n].any(), (fy64, n, center, slant)


def test_fractional_baseline_moves_the_samples(ascii_set):
    """fy != 0 adds the one row the shift can reach, and the image is neither of its whole-row neighbours"""
    gs = ascii_set.gs
    g = ascii_set.find("Serif", "f")
    scale = np.float32(40) / np.float32(int(ascii_set.g_upm[g]))
    c0, r0, w, h = tw.ex_cell(gs.boxes[g], scale, 0.0, 0, 0)
    assert tw.ex_cell(gs.boxes[g], scale, 0.0, 0, 32)[3] == h + 1
    run = rg.make_runs([(0, 1, w, h + 2, 0, 0, scale)])[0]
    img = [tw.render_run("ex", gs, rg.make_places_ex([(g, -64 * c0, -64 * r0 + d, 0.0, 0.0)]), run, 4, True) for d in (0, 32, 64)]
    assert not np.array_equal(img[1], img[0]) and not np.array_equal(img[1], img[2])
    assert np.array_equal(img[2][1:], img[0][:-1])


# ---- the slanted cell holds the glyph ----------------------------------------------------------------------------------
@pytest.mark.parametrize("slant", SLANTS)
def test_the_slanted_cell_holds_the_glyph(ascii_set, slant):
    """FR_FILL_CONSISTENT has no winding outside an outline, and the sheared outline lies inside the sheared box: two
    more columns on each side of the cell change no sample.  (Not so under the reference's rule, whose false windings on
    rows through vertices run on to the left of the glyph: that is why the cell is part of the definition.)"""
    gs = ascii_set.gs
    seg = gs.segments_per_glyph()
    rng = np.random.default_rng(int(1000 * abs(slant)) + (slant < 0))
    done = 0
    while done < 6:
        g = int(rng.integers(len(ascii_set)))
        if not seg[g]:
            continue
        scale = np.float32(int(rng.integers(16, 49))) / np.float32(int(ascii_set.g_upm[g]))
        pen_x64, fy64 = int(rng.integers(0, 64)), int(rng.integers(0, 64))
        c0, r0, w, h = tw.ex_cell(gs.boxes[g], scale, slant, pen_x64, fy64)
        run = rg.make_runs([(0, 1, w + 8, h + 2, 0, 0, scale)])[0]
        places = rg.make_places_ex([(g, pen_x64 - 64 * c0 + 64 * 4, fy64 - 64 * r0 + 64, 0.0, slant)])
        tight = tw.coverage_samples("ex", gs, places, run, 4, True, True)
        wide = tw.coverage_samples("ex", gs, places, run, 4, True, True, widen=2)
        assert tight.any()
        assert np.array_equal(tight, wide), (g, slant, float(scale))
        done += 1


def test_slant_moves_the_top_of_a_stem_to_the_right(ascii_set):
    gs = ascii_set.gs
    g = ascii_set.find("STIX", "l")
    scale = np.float32(48) / np.float32(int(ascii_set.g_upm[g]))
    run = rg.make_runs([(0, 1, 80, 64, 0, 0, scale)])[0]
    up = tw.render_run("ex", gs, rg.make_places_ex([(g, 64 * 10, 64 * 50, 0.0, 0.0)]), run, 4, True)
    ob = tw.render_run("ex", gs, rg.make_places_ex([(g, 64 * 10, 64 * 50, 0.0, 0.5)]), run, 4, True)
    cols = lambda im, row: np.nonzero(im[row])[0]
    top = min(np.nonzero(up.any(1))[0])
    assert top == min(np.nonzero(ob.any(1))[0])                      # the shear keeps every height
    assert cols(ob, top + 1).mean() > cols(up, top + 1).mean() + 10  # ~0.5 * 33 pixels of stem above the baseline
    assert abs(cols(ob, 49).mean() - cols(up, 49).mean()) < 1.5      # the baseline stays where it is


# ---- the span layout ---------------------------------------------------------------------------------------------------
def test_spans_of_one_size_are_one_layout():
    font = load_font("DejaVuSans.ttf", allow_hinted=True)
    parts = ["Tf ff", "i, fj", " Wavy"]
    gi, pen, end = font.layout("".join(parts), 21)
    gs, places, runs, w, h, colours = T.span_line(font, [(p, 21, 0.0, 0.0, (1, 2, 3)) for p in parts])
    assert len(places) == len(gi) and len(runs) == 1 and int(runs[0]["count"]) == len(gi)
    shift = int(places[0]["pen_x64"]) - int(pen[0])
    assert shift % 64 == 0 and (places["pen_x64"] - shift).tolist() == pen.tolist()
    assert len(set(places["pen_y64"].tolist())) == 1 and int(places[0]["pen_y64"]) % 64 == 0
    assert colours == [(1, 2, 3, 255)] * len(gi)
    # the same image size and pens as the line laid out in one piece
    _, p1, r1, w1, h1 = T._line(font, "".join(parts), 21)
    assert (w, h) == (w1, h1) and places["pen_x64"].tolist() == p1["pen_x64"].tolist()
    assert (places["pen_y64"] // 64).tolist() == p1["pen_y"].tolist()


def test_span_size_slant_and_rise_reach_the_placements():
    font = load_font("DejaVuSans.ttf", allow_hinted=True)
    upm = np.float32(font.information.units_per_em)
    spans = [("E = mc", 32, 0.0, 0.0, (0, 0, 0)), ("2", 16, 0.0, 14.25, (255, 0, 0, 128)), (" so", 32, 0.2, 0.0, (0, 0, 255))]
    gs, places, runs, w, h, colours = T.span_line(font, spans)
    assert places.dtype == rg.PLACE_EX_DTYPE and len(places) == 10
    assert places["scale"].tolist() == [np.float32(32) / upm] * 6 + [np.float32(16) / upm] + [np.float32(32) / upm] * 3
    assert places["slant"].tolist() == [0.0] * 7 + [np.float32(0.2)] * 3
    base = int(places[0]["pen_y64"])
    assert base % 64 == 0 and int(places[6]["pen_y64"]) == base - 912 and int(places[7]["pen_y64"]) == base
    _, _, e0 = font.layout("E = mc", 32)
    _, _, e1 = font.layout("2", 16)
    shift = int(places[0]["pen_x64"])
    assert int(places[6]["pen_x64"]) == shift + e0 and int(places[7]["pen_x64"]) == shift + e0 + e1
    assert colours[6] == (255, 0, 0, 128) and colours[9] == (0, 0, 255, 255)
    # the image is the union of the cells: every cell inside, and some cell on each edge
    local = {int(g): k for k, g in enumerate(sorted({int(g) for t, s, *_ in spans for g in font.layout(t, s)[0]}))}
    seg = gs.segments_per_glyph()
    cells = [T.instance_cell_ex(gs.boxes[int(p["glyph"])], p["scale"], p["slant"], int(p["pen_x64"]), int(p["pen_y64"]))
             for p in places if seg[int(p["glyph"])]]
    assert len(local) == len(gs.boxes)
    assert min(c[1] for c in cells) == 0 and max(c[1] + c[3] for c in cells) == h
    assert min(c[0] for c in cells) >= 0 and max(c[0] + c[2] for c in cells) == w
    for p in places:                                                   # the twin's cell is the package's
        args = (gs.boxes[int(p["glyph"])], p["scale"], p["slant"], int(p["pen_x64"]), int(p["pen_y64"]))
        assert T.instance_cell_ex(*args) == tw.ex_cell(*args)


def test_view_line_places_the_zoomed_line():
    font = load_font("DejaVuSans.ttf", allow_hinted=True)
    gi, pen, _ = font.layout("Tf fj", 16)
    gs, places, runs = T.view_line(font, "Tf fj", 16, 1.5, 10.3, 20.75, 200, 64)
    assert places["pen_y64"].tolist() == [1328] * 5 and places["scale"].tolist() == [0.0] * 5
    assert places["pen_x64"].tolist() == [int(np.floor(64 * 10.3 + 1.5 * int(p) + 0.5)) for p in pen]
    assert runs[0]["scale"] == np.float32(24) / np.float32(font.information.units_per_em)
    assert (int(runs[0]["w"]), int(runs[0]["h"])) == (200, 64)
    assert T.view_line(font, "", 16, 1.0, 0, 0, 10, 10) is None and T.view_line(font, "a", 16, 1.0, 0, 0, 0, 10) is None


# ---- validation of the new Python arguments (all raised before anything touches a device) --------------------------------
def test_python_argument_validation():
    font = load_font("DejaVuSans.ttf", allow_hinted=True)
    for bad in (4.5, -4.01, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            T.render_text(font, "a", 16, slant=bad)
        with pytest.raises(ValueError):
            T.span_line(font, [("a", 16, bad, 0.0, (0, 0, 0))])
        with pytest.raises(ValueError):
            T.view_line(font, "a", 16, 1.0, 0.0, 0.0, 10, 10, slant=bad)
    with pytest.raises(ValueError):
        T.span_line(font, [("a", 16, 0.0, (0, 0, 0))])
    with pytest.raises(ValueError):
        T.span_line(font, [("a", 16.5, 0.0, 0.0, (0, 0, 0))])
    with pytest.raises(ValueError):
        T.span_line(font, [("a", 16, 0.0, float("nan"), (0, 0, 0))])
    with pytest.raises(ValueError):
        T.span_line(font, [("a", 16, 0.0, 0.0, (0, 0, 256))])
    for zoom in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            T.view_line(font, "a", 16, zoom, 0.0, 0.0, 10, 10)
    with pytest.raises(ValueError):
        T.view_line(font, "a", 16, 1.0, float("nan"), 0.0, 10, 10)
    with pytest.raises(ValueError):
        T.view_line(font, "a", 16, 1.0, 0.0, 0.0, 70000, 10)
    assert T.span_line(font, []) is None
    assert rg.make_places_ex([(1, 2, 3, 0.5, 0.25)]).tobytes() == np.array([1, 2, 3], "<i4").tobytes() + np.array([0.5, 0.25], "<f4").tobytes()

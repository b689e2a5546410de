"""FR_FILL_CONSISTENT's CPU twin (tests/fill_rule_ref.py) against the oracle and against hand-counted cases.  No GPU."""
import numpy as np
import pytest

import fill_rule_ref as FR
import oracle_lib as O
from font_renderer_amd.glyph import Box, Contour, Glyph, GlyphSet

SIZES = (64, 33, 100, 17)          # renderGlyph sizes of the fixture's checks (tests/test_zig_vectors.py)


def _flat(glyph):
    gs = GlyphSet([glyph])
    return gs.points_xy, gs.contour_start


@pytest.fixture(scope="module")
def ascii_fill(ascii_set):
    """twin windings of every fixture glyph at every size: {(i, size): (cell, windings)}"""
    res = {}
    for i in range(len(ascii_set)):
        g = ascii_set.glyph(i)
        pts, cs = _flat(g)
        for size in SIZES:
            cell = FR.glyph_dims(g.box.as_array(), int(ascii_set.g_upm[i]), size)
            res[(i, size)] = (cell, FR.render_cell(pts, cs, *cell, FR.WINDING_I16))
    return res


def _far_rows(pts, cs, cy):
    ends, margin = FR.piece_end_heights(pts, cs)
    if len(ends) == 0:
        return np.ones(len(cy), bool)
    return (np.abs(cy.astype(np.float64)[:, None] - ends[None, :]) > margin[None, :]).all(axis=1)


def test_equals_the_reference_away_from_piece_ends(oracle, ascii_set, ascii_fill):
    """(a) wherever the ray is clear of every piece-end height the two rules cross the same pieces — clear: more than
    2^-8 font units, or more than the blur of the reference's own rounded acceptance where that is wider
    (fill_rule_ref.piece_end_heights; a nearly straight quadratic blurs its ends by up to ~0.5 font units) — the twin equals the oracle's binary32 winding (n = 1) and its 16-sample coverage (n = 4, on pixels all
    of whose sample rows are that far)"""
    compared = 0
    for (i, size), (cell, wd) in ascii_fill.items():
        g = ascii_set.glyph(i)
        pts, cs = _flat(g)
        ref = oracle.render_cell(g, *cell, O.WINDING_I16)
        _, cy = FR.sample_axes(*cell)
        far = _far_rows(pts, cs, cy)
        assert np.array_equal(wd[far], ref[far]), (i, size)
        compared += int(far.sum()) * cell[2]
        if size in (33, 17):
            cov = FR.render_cell(pts, cs, *cell, FR.COVERAGE_U8, 4, True)
            refc = oracle.render_cell(g, *cell, O.COVERAGE_U8, 4, True)
            _, cy4 = FR.sample_axes(*cell, 4, True)
            far4 = _far_rows(pts, cs, cy4).reshape(-1, 4).all(axis=1)
            assert np.array_equal(cov[far4], refc[far4]), (i, size)
    assert compared > 1_000_000


def test_no_negative_winding_on_the_fixture(ascii_fill, ascii_set):
    """(b) every outline of the fixture is clockwise-outer, as TrueType's (windings 0 / 1 / 2 ...): under the consistent rule no
    sample of any of its 190 glyphs at any of the four sizes has a negative winding"""
    bad = [(i, s) for (i, s), (_, wd) in ascii_fill.items() if (wd < 0).any()]
    assert bad == [], bad


def test_stix_A_baseline(oracle, ascii_set):
    """(c) STIX 'A' at renderGlyph size 64: the reference puts -1 x28 and -2 x1 on row 44 (the baseline, y = 0); the
    consistent rule has none there, and every pixel off row 44 is the reference's"""
    i = ascii_set.find("STIX", "A")
    g = ascii_set.glyph(i)
    pts, cs = _flat(g)
    wd = FR.render_glyph(pts, cs, g.box.as_array(), 1000, 64, FR.WINDING_I16)
    ref = oracle.render_cell(g, *FR.glyph_dims(g.box.as_array(), 1000, 64), O.WINDING_I16)
    assert wd.shape == (45, 47)
    assert (ref[44] < 0).sum() == 29
    assert not (wd[44] < 0).any()
    assert np.array_equal(np.delete(wd, 44, axis=0), np.delete(ref, 44, axis=0))


def _line_contour(xy):
    """closed polygon of on-curve points -> contour with midpoint controls (a == 0 segments)"""
    pts = []
    n = len(xy)
    for k in range(n):
        (x0, y0), (x1, y1) = xy[k], xy[(k + 1) % n]
        pts += [(x0, y0), ((x0 + x1) // 2, (y0 + y1) // 2)]
    pts.append(xy[0])
    return Contour(np.array(pts, np.int16))


def _w(glyph, x, y):
    pts, cs = _flat(glyph)
    return int(FR.winding_fill(pts, cs, np.float32(x), np.float32(y)))


def test_hand_made_cases(oracle):
    """(d) the four configurations the reference miscounts, each with the count written down"""
    # (outer outlines run clockwise, as TrueType's: winding +1 inside)
    # a diamond whose ray through the side vertices (y = 0) is inside: exactly 1; its bottom vertex is an extremum,
    # crossed twice with opposite signs; its top vertex is the top end of both pieces, never crossed
    diamond = Glyph(Box(-20, -20, 20, 20), [_line_contour([(0, -20), (-20, 0), (0, 20), (20, 0)])])
    assert _w(diamond, -10, 0) == 1 and _w(diamond, 0, 0) == 1 and _w(diamond, 10, 0) == 1
    assert _w(diamond, -30, 0) == 0 and _w(diamond, 30, 0) == 0
    assert _w(diamond, 0, 20) == 0 and _w(diamond, 0, -20) == 0 and _w(diamond, 0, -19) == 1
    # a square with the ray along its bottom and top edges: the bottom row is inside, the top row outside
    square = Glyph(Box(0, 0, 20, 20), [_line_contour([(0, 0), (0, 20), (20, 20), (20, 0)])])
    assert _w(square, 10, 0) == 1 and _w(square, 10, 20) == 0 and _w(square, 10, 10) == 1
    assert _w(square, -1, 0) == 0 and _w(square, 25, 0) == 0
    # the reference rejects t = 1 of the right side at y = 0 and calls the bottom row outside
    assert oracle.winding_at(square, 10, 0) == 0
    # the same square with a collinear extra vertex on its right side
    square5 = Glyph(Box(0, 0, 20, 20), [_line_contour([(0, 0), (0, 20), (20, 20), (20, 10), (20, 0)])])
    for y in (0, 5, 10, 15, 19.5):
        assert _w(square5, 10, y) == 1, y
    assert _w(square5, 10, 20) == 0 and _w(square5, 25, 10) == 0
    # a tangent extremum: a quadratic bump whose top t_v = 1/2 sits at y = 10; a ray at y = 10 crosses it 0 times net
    # (two pieces, -1 and +1), above it never, below it twice (net 0 for the open bump, the closing line adds 1)
    bump = Glyph(Box(0, 0, 40, 10), [Contour(np.array([(0, 0), (20, 20), (40, 0), (20, 0), (0, 0)], np.int16))])
    assert _w(bump, 20, 10) == 0 and _w(bump, 20, 10.5) == 0
    assert _w(bump, 20, 5) == 1 and _w(bump, 20, 0) == 1 and _w(bump, -5, 5) == 0
    assert _w(bump, 20, -0.5) == 0

"""Row cuts (option "row_cuts"): the fast kernels' set-up reads the class of a sample row off two
heights per candidate root that fr_glyphset_create found once.  Here: the cuts against the acceptance expression at
every row of many cells (fr_selftest_row_cuts), rows that lie exactly on a cut, both ways through every set-up, and the
single-image path that has no table.  Byte equality with the CPU references throughout, over sentinel-filled arrays."""
import numpy as np
import pytest

import fill_rule_ref as FR
import font_renderer_amd as fr
import oracle_lib as O
from font_renderer_amd import render_glyph as rg
from font_renderer_amd.atlas import cell_jobs, glyph_dims_jobs
from font_renderer_amd.glyph import Box, Contour, Glyph, GlyphSet
from font_renderer_amd.synth import comb_glyph, synth_glyphset

pytestmark = pytest.mark.gpu
SENT = 0x5b
OMODE = {fr.FR_WINDING_I16: O.WINDING_I16, fr.FR_GRAY_DEBUG: O.GRAY_DEBUG, fr.FR_COVERAGE_U8: O.COVERAGE_U8}
CORNER, CENTER = fr.FR_SAMPLE_CORNER, fr.FR_SAMPLE_CENTER


def _glyph(contours):
    cs = [Contour(np.array(c, np.int16)) for c in contours]
    allp = np.concatenate([c.points for c in cs])
    return Glyph(Box(int(allp[:, 0].min()), int(allp[:, 1].min()), int(allp[:, 0].max()), int(allp[:, 1].max())), cs)


def _live_candidates(gs):
    """per glyph: the candidate roots the set-up does not discard from the control points alone (record_prep,
    fr_records.hpp) — a == 0: the one root unless p2y == p0y; else the far-side root unless t_v = b / a >= 1 and the
    near-side root unless t_v < 0.  What fr_selftest_row_cuts compares at every row."""
    out = np.zeros(len(gs), np.int64)
    pts = gs.points_xy.astype(np.int64)
    for g in range(len(gs)):
        for c in range(int(gs.glyph_start[g]), int(gs.glyph_start[g + 1])):
            y = pts[int(gs.contour_start[c]):int(gs.contour_start[c + 1]), 1]
            if len(y) < 3:
                continue
            p0, p1, p2 = y[0:-1:2], y[1::2], y[2::2]
            a, b = p0 - 2 * p1 + p2, p0 - p1
            lin = a == 0
            tv_ge1 = np.where(a > 0, b >= a, b <= a)
            tv_lt0 = b * a < 0
            for root in (0, 1):
                far = (a > 0) if root == 0 else (a < 0)
                live = np.where(lin, (p2 != p0) if root == 0 else False, np.where(far, ~tv_ge1, ~tv_lt0))
                out[g] += int(live.sum())
    return out


def _selftest(dgs, gs, jobs, live=None):
    """all six sample grids: 0 mismatches, and as many pairs as the jobs imply"""
    live = _live_candidates(gs) if live is None else live
    assert live.sum() > 0
    for n in (1, 2, 4):
        want = int((live[jobs["glyph"].astype(np.int64)] * jobs["h"].astype(np.int64) * n).sum())
        for phase in (CORNER, CENTER):
            pairs, bad, first = dgs.selftest_row_cuts(jobs, n, phase)
            assert bad == 0, (n, phase, bad, "first (job, candidate, row):", first, jobs[first[0]])
            assert pairs == want and pairs > 0, (n, phase, pairs, want)


def test_selftest_ascii_fixture_at_renderglyph_dims(ctx, ascii_set):
    """every fixture glyph at six font sizes, cells of exactly renderGlyph's image size"""
    gs = ascii_set.gs
    live = _live_candidates(gs)
    dgs = fr.DeviceGlyphSet(ctx, gs)
    try:
        for size in (9, 17, 33, 64, 100, 200):
            jobs, _ = glyph_dims_jobs(gs, size, ascii_set.g_upm, 4096)
            assert len(jobs) == len(gs)
            _selftest(dgs, gs, jobs, live)
    finally:
        dgs.close()


@pytest.mark.parametrize("segments", [16, 128, 256, 512, "comb"])
def test_selftest_synthetic_glyphs(ctx, segments):
    """8 synthetic glyphs per segment count (every set-up: one wave, two waves, the general one) and a comb of straight
    edges, in 64^2 and 256^2 cells"""
    if segments == "comb":
        cs, box = comb_glyph(12)
        gs = GlyphSet.from_arrays(cs[0], np.array([0, len(cs[0])], np.uint32), np.array([0, 1], np.uint32), box[None, :])
    else:
        gs = synth_glyphset(8, segments)
    dgs = fr.DeviceGlyphSet(ctx, gs)
    try:
        for cell in (64, 256):
            _selftest(dgs, gs, cell_jobs(gs, cell, cell, 2048, 4))
    finally:
        dgs.close()


def _extreme_set():
    """coordinates at the ends of i16, and a glyph of a few units around the origin (for the largest scales)"""
    m, M = -32768, 32767
    big = _glyph([[(m, m), (m, 0), (m, M), (0, M), (M, M), (M, 1), (M, m), (0, m), (m, m)],                 # the square of all i16
                  [(m, 0), (-5, M), (M, 3), (7, m), (m, 0)],                                                # steep parabolas
                  [(-3, m), (M, -32767), (-2, M), (m, 32766), (-3, m)]])
    small = _glyph([[(-3, -2), (0, 3), (3, -2), (0, -2), (-3, -2)], [(-1, 0), (0, 2), (1, 0), (0, -1), (-1, 0)]])
    return GlyphSet([big, small])


def test_selftest_extreme_coordinates_and_scales(ctx):
    """i16-extreme control points; scales 2^-20 and 2^20 (the ends of what a plan accepts), the two neighbours of a
    power of two, and a scale with a full significand"""
    gs = _extreme_set()
    f32 = np.float32
    rows = []
    for g in (0, 1):
        rows.append((g, -2, 2, 4, 4, 0, 0, f32(2.0 ** -20)))                       # the whole glyph inside one pixel
        rows.append((g, -300, 260, 600, 520, 0, 0, f32(2.0 ** -7)))
        for s in (np.nextafter(f32(0.5), f32(0)), np.nextafter(f32(0.5), f32(1)), f32(0.0997331), f32(3.1415927)):
            top = int(np.ceil(float(gs.boxes[g][3]) * float(s))) + 3
            rows.append((g, -40, min(top, 1 << 22), 80, 300, 0, 0, s))
    # 2^20 pixels per font unit: windows of 64 rows around heights -2, 0 and 3 of the small glyph (|y| 2^20 <= 2^22)
    for y in (-2, 0, 3):
        rows.append((1, -32, y * (1 << 20) + 32, 64, 64, 0, 0, f32(2.0 ** 20)))
    rows.append((0, -32, 32, 64, 64, 0, 0, f32(2.0 ** 20)))
    jobs = rg.make_jobs(rows)
    dgs = fr.DeviceGlyphSet(ctx, gs)
    try:
        _selftest(dgs, gs, jobs)
    finally:
        dgs.close()


def test_selftest_tall_cells(ctx):
    """a cell of 2 048 sample rows (512 pixel rows x 4, and 2 048 x 1), and taller"""
    gs = synth_glyphset(3, 128)
    jobs = rg.make_jobs([(0, 0, 512, 512, 512, 0, 0, np.float32(0.25)), (1, 0, 2048, 64, 2048, 0, 0, np.float32(1.0)),
                         (2, -7, 1031, 64, 1024, 0, 0, np.float32(0.503))])
    dgs = fr.DeviceGlyphSet(ctx, gs)
    try:
        _selftest(dgs, gs, jobs)
    finally:
        dgs.close()


def _render(ctx, dgs, jobs, mode, shape, n, phase, flags=0):
    out = np.full(shape, SENT, np.int16 if mode == fr.FR_WINDING_I16 else np.uint8)
    return rg.render_batch(dgs, jobs, mode, out, n, phase, flags)


def _oracle(oracle, gs, jobs, mode, shape, n, phase):
    out = np.full(shape, SENT, np.int16 if mode == fr.FR_WINDING_I16 else np.uint8)
    return oracle.render_batch(gs, jobs, OMODE[mode], out, n, phase == CENTER, 16)


def _both_ways(ctx, dgs, jobs, mode, shape, n, phase, flags=0):
    """the render with row_cuts = 1 and = 0, and the plan's description under each"""
    got = {}
    try:
        for cuts in (1, 0):
            ctx.set_option("row_cuts", cuts)
            plan = fr.Plan(dgs, jobs, mode, n, phase, flags)
            desc, st = plan.describe(), plan.stats()
            plan.close()
            got[cuts] = (_render(ctx, dgs, jobs, mode, shape, n, phase, flags), desc, st)
    finally:
        ctx.set_option("row_cuts", 1)
    assert got[1][1] == got[0][1], (got[1][1], got[0][1])
    assert np.array_equal(got[1][0], got[0][0]), (got[1][1], np.argwhere(got[1][0] != got[0][0])[:4].tolist())
    return got[1]


# on-curve points and vertex heights are integers: with corner samples and a power-of-two scale, sample rows pass
# exactly through p0y, p2y and the vertex of every segment — the heights where the cuts sit
ON_CUT_GLYPHS = [
    [[(0, 0), (8, 8), (16, 0), (8, 0), (0, 0)]],                                                        # arch: vertex at 4
    [[(0, 8), (4, 12), (8, 16), (12, 12), (16, 8), (12, 4), (8, 0), (4, 4), (0, 8)]],                 # diamond of lines
    [[(0, 0), (4, 12), (20, 8), (20, 2), (20, -4), (10, -12), (0, -4), (0, -2), (0, 0)]],             # vertices at 9 and -8
    [[(0, 0), (8, -8), (16, 0), (16, 8), (16, 16), (8, 24), (0, 16), (0, 8), (0, 0)]],                # valley and hill
]


def test_rows_exactly_on_a_cut(ctx, oracle, ascii_set):
    gs = GlyphSet([_glyph(c) for c in ON_CUT_GLYPHS])
    rows, x = [], 0
    for s in (1.0, 2.0, 0.5, 4.0):
        for g in range(len(gs)):
            b = gs.boxes[g].astype(np.float64)
            w, h = int((b[2] - b[0]) * s) + 9, int((b[3] - b[1]) * s) + 9
            rows.append((g, int(np.floor(b[0] * s)) - 4, int(np.ceil(b[3] * s)) + 4, w, h, x, 1, np.float32(s)))
            x += w + 1
    jobs = rg.make_jobs(rows)
    shape = (int(jobs["h"].max()) + 2, x)
    dgs = fr.DeviceGlyphSet(ctx, gs)
    try:
        for mode, n in ((fr.FR_WINDING_I16, 1), (fr.FR_COVERAGE_U8, 4)):
            got, desc, st = _both_ways(ctx, dgs, jobs, mode, shape, n, CORNER)
            assert st["jobs_general"] == 0, desc
            want = _oracle(oracle, gs, jobs, mode, shape, n, CORNER)
            assert np.array_equal(got, want), (mode, desc, np.argwhere(got != want)[:4].tolist())
            assert (got[0] == SENT).all() and (want != SENT).any() and (want[want != SENT] != 0).any()
    finally:
        dgs.close()
    # STIX 'A' at size 64: the reference's 29 negative windings on row 44 come from rows on a vertex height
    i = ascii_set.find("STIX", "A")
    gs = GlyphSet([ascii_set.glyph(i)])
    jobs, H = glyph_dims_jobs(gs, 64, int(ascii_set.g_upm[i]), 64)
    assert (int(jobs["w"][0]), int(jobs["h"][0])) == (47, 45)
    dgs = fr.DeviceGlyphSet(ctx, gs)
    try:
        for mode, n in ((fr.FR_WINDING_I16, 1), (fr.FR_COVERAGE_U8, 4)):
            got, desc, st = _both_ways(ctx, dgs, jobs, mode, (H + 1, 64), n, CORNER)
            assert st["jobs_general"] == 0, desc
            assert np.array_equal(got, _oracle(oracle, gs, jobs, mode, got.shape, n, CORNER)), (mode, desc)
            if mode == fr.FR_WINDING_I16:
                assert (got[44, :47] < 0).sum() == 29
    finally:
        dgs.close()


@pytest.mark.parametrize("segments", [20, 50, 128, 300, 600])
def test_both_ways_through_every_setup(ctx, oracle, segments):
    """glyphs for the one-wave, the two-wave and the general set-up (4, 8 and 16 candidates per lane), in 64 x 64 and
    ragged 47 x 45 cells, through cov4_kernel (4 x 4 and 2 x 2 samples) and win1_kernel (gray map, windings): row_cuts 1
    and 0 render the same bytes, the oracle's, from the same launches; under FR_FILL_CONSISTENT the cuts are present and
    not used, and the bytes are the twin's"""
    gs = synth_glyphset(2, segments)
    full = cell_jobs(gs, 64, 64, 2048, 2)
    ragged = full.copy()
    ragged["w"], ragged["h"] = 47, 45
    dgs = fr.DeviceGlyphSet(ctx, gs)
    try:
        for jobs in (full, ragged):
            for mode, n, phase in ((fr.FR_COVERAGE_U8, 4, CENTER), (fr.FR_COVERAGE_U8, 2, CENTER),
                                   (fr.FR_GRAY_DEBUG, 1, CORNER), (fr.FR_WINDING_I16, 1, CORNER)):
                got, desc, st = _both_ways(ctx, dgs, jobs, mode, (65, 128), n, phase)
                assert st["jobs_general"] == 0 and ("cov4_kernel" if mode == fr.FR_COVERAGE_U8 else "win1_kernel") in desc, desc
                want = _oracle(oracle, gs, jobs, mode, (65, 128), n, phase)
                assert np.array_equal(got, want), (mode, n, desc, np.argwhere(got != want)[:4].tolist())
                assert (got[64] == SENT).all() and (want[:45, :47] != 0).any()
        for mode, n, phase in ((fr.FR_COVERAGE_U8, 2, CENTER), (fr.FR_GRAY_DEBUG, 1, CORNER)):
            got, desc, st = _both_ways(ctx, dgs, ragged, mode, (65, 128), n, phase, fr.FR_FILL_CONSISTENT)
            assert st["jobs_general"] == 0, desc
            want = FR.render_batch(gs, ragged, mode, np.full((65, 128), SENT, np.uint8), n, phase == CENTER)
            assert np.array_equal(got, want), (mode, n, desc, np.argwhere(got != want)[:4].tolist())
    finally:
        dgs.close()


def test_single_image_path_has_no_table(ctx, oracle, ascii_set):
    """fr.renderGlyph dresses its arena as a glyph set per call and passes no cuts: still the oracle's image"""
    for name, size in (("A", 64), ("g", 33), ("A", 17)):
        i = ascii_set.find("STIX", name)
        g, upm = ascii_set.glyph(i), int(ascii_set.g_upm[i])
        im = fr.renderGlyph(g, fr.FontInformation(upm), size, ctx=ctx)
        assert np.array_equal(im.as_2d(), oracle.render_glyph(g, upm, size)), (name, size)

"""The pair walk of cov4_kernel and the set-up it shares with win1_kernel, where their arithmetic takes a shortcut:

  * a job whose scale is a power of two gets its ray heights and its cx table by a multiply, every other scale by the
    IEEE division (ScaleDiv, csrc/fr_device.hpp) — powers of two, their neighbours and both ends of the range a plan accepts;
  * the walk's markers, row offsets and trip counters are pre-scaled byte offsets (csrc/fr_cov4_kernel.inc) — record
    ranges that start before and end after a band, partial bands, more pairs than one chunk holds, the two-records-per-lane
    layout inside the four-records instance, the instances that walk a band three times, the FR_FILL_CONSISTENT twin;
  * the toggle walk's signs — rows of more than 16 crossings, windings of +-2, the second difference of a pixel in byte 3.

A few small cells per case; every render goes into a sentinel-filled array and equals the CPU reference over the whole
array: the C oracle, or the numpy twin of FR_FILL_CONSISTENT (tests/fill_rule_ref.py) for the twin instance."""
import functools

import numpy as np
import pytest

import fill_rule_ref as FR
import font_renderer_amd as fr
import instance_cases as IC
from font_renderer_amd import render_glyph as rg
from font_renderer_amd.glyph import Box, Contour, Glyph, GlyphSet
from font_renderer_amd.synth import comb_glyph, stroke_glyphset, synth_glyphset

pytestmark = pytest.mark.gpu
SENTINEL = 0x5b
HEADLINE = "fr::cov4_kernel<4, 32, 4, 4>"


# ---- helpers --------------------------------------------------------------------------------------------------------
def _place(rows, gap=5):
    """(glyph, min_x, max_y, w, h, scale) rows side by side at odd out_x -> (jobs, shape), sentinels on every side"""
    out, x = [], 3
    for g, min_x, max_y, w, h, s in rows:
        out.append((g, min_x, max_y, w, h, x, 2, np.float32(s)))
        x += w + gap + (w + gap) % 2
    stride = x + 2 + (1 if (x + 2) % 16 == 0 else 0)
    return rg.make_jobs(out), (2 + max(r[4] for r in rows) + 3, stride)


def _render_both(ctx, oracle, gs, jobs, shape, mode, n, center, fill=0):
    """-> (got, ref, describe()) of one plan; ref: the oracle (fill = 0) or the numpy twin of the consistent fill rule"""
    dt = np.int16 if mode == fr.FR_WINDING_I16 else np.uint8
    phase = fr.FR_SAMPLE_CENTER if center else fr.FR_SAMPLE_CORNER
    flags = fr.FR_FILL_CONSISTENT if fill else 0
    dgs = fr.DeviceGlyphSet(ctx, gs)
    try:
        plan = fr.Plan(dgs, jobs, mode, n, phase, flags)
        st, desc = plan.stats(), plan.describe()
        plan.close()
        assert st == {"jobs_cov4": len(jobs), "jobs_general": 0}, (st, desc)      # the fast kernels, every job
        got = rg.render_batch(dgs, jobs, mode, np.full(shape, SENTINEL, dt), n, phase, flags)
    finally:
        dgs.close()
    if fill:
        ref = FR.render_batch(gs, jobs, mode, np.full(shape, SENTINEL, dt), n, center)
    else:
        ref = oracle.render_batch(gs, jobs, mode, np.full(shape, SENTINEL, dt), n, center, 16)
    return got, ref, desc


def _same(got, ref, what):
    bad = np.argwhere(got != ref)
    assert bad.size == 0, (what, len(bad), "first (row, col):", bad[:4].tolist(),
                           "got", [int(got[tuple(b)]) for b in bad[:4]], "want", [int(ref[tuple(b)]) for b in bad[:4]])
    assert (ref != SENTINEL).any() and (ref == SENTINEL).any()


def _first(desc):
    return desc.split("; ")[0].rsplit(" x", 1)[0]


def _poly_glyph(polys):
    """closed polygons of integer points -> a glyph of straight segments (truncated midpoints as control points)"""
    cs = []
    for poly in polys:
        poly = np.array(poly, np.int64)
        pts = np.empty((2 * len(poly) + 1, 2), np.int64)
        pts[0:-1:2] = poly
        pts[1:-1:2] = IC._div_trunc2(poly + np.roll(poly, -1, 0))
        pts[-1] = poly[0]
        cs.append(pts.astype(np.int16))
    allp = np.concatenate(cs)
    return Glyph(Box(int(allp[:, 0].min()), int(allp[:, 1].min()), int(allp[:, 0].max()), int(allp[:, 1].max())),
                 [Contour(c) for c in cs])


@functools.lru_cache(maxsize=None)
def _synth_with_roots(segs, lo, hi, first_index):
    """the first synth glyph of `segs` segments from `first_index` on whose candidate-root bound lies in [lo, hi]"""
    for k in range(64):
        gs = synth_glyphset(1, segs, first_index=first_index + k)
        if lo <= IC.root_bound(IC.glyph_segments(gs, 0)) <= hi:
            return gs.glyph(0)
    raise ValueError(f"no synth glyph of {segs} segments with {lo} .. {hi} candidate roots")


@functools.lru_cache(maxsize=None)
def _of_class(make, segs, rc, first_index):
    """the first glyph of the generator, from `first_index` on, that the host rules put into record class rc"""
    for k in range(64):
        gs = make(1, segs, first_index=first_index + k)
        sg = IC.glyph_segments(gs, 0)
        if IC.fast_class(4, 256, 64, len(sg), IC.root_bound(sg), IC.ray_bound(sg)) == 9 + rc:
            return gs.glyph(0)
    raise ValueError(f"no {make.__name__}({segs}) glyph of record class {rc}")


# ---- scale classes --------------------------------------------------------------------------------------------------
# powers of two (the multiply), neighbours that must take the division, and both ends of [2^-20, 2^20] (fr_plan_create)
P2 = [2.0 ** -3, 2.0 ** -4, 1.0]
NEAR = [100.0 / 2048.0, float(np.nextafter(np.float32(2.0 ** -3), np.float32(1.0)))]
ENDS = [2.0 ** -20, 2.0 ** 20]


@functools.lru_cache(maxsize=None)
def _scale_glyphs():
    """24, 50 and 128 segments — the one-wave, two-wave and general set-up (fr_c4.hpp) — and a curved glyph whose outline
    runs through the on-curve point (1, -1) with the origin just inside: the only place where a cell at scale 2^20 (4 units
    across at most: pixel coordinates stay within +-2^22) or at 2^-20 can see it"""
    gl = [synth_glyphset(1, sg, first_index=40 + sg).glyph(0) for sg in (24, 50, 128)]
    pts = np.array([(-1000, -800), (-300, -700), (1, -1), (200, 600), (-500, 1000), (-1200, 300), (-1000, -800)], np.int16)
    gl.append(Glyph(Box(-1200, -800, 200, 1000), [Contour(pts)]))
    return GlyphSet(gl)


def _scale_rows(gs, s, w, h):
    s32 = float(np.float32(s))
    if s == ENDS[1]:                      # the point (1, -1) at pixel (30, 18) of the cell
        return [(3, (1 << 20) - 30, -(1 << 20) + 18, w, h, s32)]
    if s == ENDS[0]:                      # the whole glyph between two samples; pixel (20, 15) is the sample at the origin
        return [(3, -20, 15, w, h, s32)]
    rows = []
    for g in range(3):                    # an on-curve point of the glyph at pixel (20, 15) of its cell
        p = gs.glyph(g).contours[0].points[0]
        rows.append((g, int(np.floor(float(p[0]) * s32)) - 20, int(np.ceil(float(p[1]) * s32)) + 15, w, h, s32))
    return rows


@pytest.mark.parametrize("s", P2 + NEAR + ENDS, ids=lambda s: f"{s:.9g}")
def test_scale_classes(ctx, oracle, s):
    """cov4 (NS 4 and 2, centre phase) and win1 (corner phase, gray map and int16 windings) on cells around an on-curve
    point of a 24-, a 50- and a 128-segment glyph; at the ends of the range on the glyph through (1, -1)"""
    gs = _scale_glyphs()
    jobs, shape = _place(_scale_rows(gs, s, 70, 37))
    for mode, n, center in ((fr.FR_COVERAGE_U8, 4, True), (fr.FR_COVERAGE_U8, 2, True),
                            (fr.FR_GRAY_DEBUG, 1, False), (fr.FR_WINDING_I16, 1, False)):
        got, ref, desc = _render_both(ctx, oracle, gs, jobs, shape, mode, n, center)
        _same(got, ref, (s, mode, n, desc))
        # (at 2^-20 the centre-phase samples all lie 2^17 units and more from the glyph: an empty cell is the right answer)
        if not (s == ENDS[0] and center):
            cell = ref[2:2 + 37, 3:3 + 70]
            assert (cell != cell[0, 0]).any(), (s, mode, n, "the cell shows no outline")


# ---- the headline instance ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("segs", [96, 112, 128])
def test_headline_instance_bands_and_row_offsets(ctx, oracle, segs):
    """glyphs of 96 - 128 segments with 129 .. 256 candidate roots in 144-pixel cells (WLOG = 4) of 80 rows (five bands)
    and of 77 (the last band partial), cut out of the MIDDLE of the glyph at 256 and at ~ 410 pixels per em: record
    ranges start above the cell (row 0 of band 0), run through several bands (every band starts at a multiple of 64
    sample rows) and end below it.  A power-of-two scale and one that divides."""
    g = _synth_with_roots(segs, 129, 256, 500 + segs)
    gs = GlyphSet([g])
    b = g.box
    rows = []
    for s, h in ((1.0 / 8, 80), (1.0 / 8, 77), (0.2003, 80), (0.2003, 77)):
        s32 = float(np.float32(s))
        mid_y = int(np.ceil((b.y_min + b.y_max) / 2 * s32)) + h // 2
        rows.append((0, int(np.floor(b.x_min * s32)) - 3, mid_y, 144, h, s32))
    jobs, shape = _place(rows)
    got, ref, desc = _render_both(ctx, oracle, gs, jobs, shape, fr.FR_COVERAGE_U8, 4, True)
    assert desc.split("; ")[0] == f"{HEADLINE} x{len(jobs)}", desc
    _same(got, ref, (segs, desc))
    # the outline enters through the cell's first row and leaves through its last: ranges are cut by the cell
    for j in jobs:
        cell = ref[2:2 + int(j["h"]), int(j["out_x"]):int(j["out_x"]) + 144]
        assert cell[0].any() and cell[-1].any()


def test_chunk_boundary(ctx, oracle):
    """a stroke-dense glyph in a 256 x 256 cell: more (record, row) pairs in a band than one chunk of 448 holds, so the
    markers and the running record index cross a chunk.  Every segment meets every sample row strictly between its end
    heights, so the pairs of the cell's 16 bands number at least the sum below: more than 448 per band on average."""
    gs = GlyphSet([_of_class(stroke_glyphset, 128, 1, 77), _of_class(stroke_glyphset, 128, 1, 90)])
    s32 = float(np.float32(1.0 / 8))
    rows = [(g, 0, 256, 256, 256, s32) for g in range(2)]
    for g in range(2):
        seg = IC.glyph_segments(gs, g)
        pairs = sum(max(0, int(abs(int(p2y) - int(p0y)) * s32 * 4) - 1) for (_, p0y), _, (_, p2y) in seg.tolist())
        assert pairs > 16 * 448, pairs
    jobs, shape = _place(rows)
    got, ref, desc = _render_both(ctx, oracle, gs, jobs, shape, fr.FR_COVERAGE_U8, 4, True)
    assert desc.split("; ")[0] == f"{HEADLINE} x2", desc
    _same(got, ref, desc)


def test_runtime_record_classes(ctx, oracle):
    """inside the four-records-per-lane instance: a glyph that leaves <= 128 records (64 segments, sent there by its
    crossings per ray: the walk then keeps two records per lane) and one that leaves more (>= 170 candidate roots, the
    whole glyph inside the cell so that nearly all of them have rows)"""
    few = _of_class(stroke_glyphset, 64, 1, 31)
    many = _synth_with_roots(128, 170, 256, 900)
    assert IC.root_bound(IC.glyph_segments(GlyphSet([few]), 0)) <= 128
    for g in (few, many):
        gs = GlyphSet([g])
        jobs, shape = _place([(0, 0, 256, 256, 256, 0.125), (0, 0, 206, 206, 206, float(np.float32(0.1)))])
        got, ref, desc = _render_both(ctx, oracle, gs, jobs, shape, fr.FR_COVERAGE_U8, 4, True)
        assert desc.split("; ")[0] == f"{HEADLINE} x2", desc
        _same(got, ref, desc)


# ---- the shared body: three walks per band, and the consistent-fill twin ------------------------------------------------
@pytest.mark.parametrize("make,segs,rpl", [(synth_glyphset, 300, 8), (synth_glyphset, 600, 16), (stroke_glyphset, 600, 16)],
                         ids=["synth300", "synth600", "stroke600"])
def test_split_instances(ctx, oracle, make, segs, rpl):
    """one cell each of a 300- and a 600-segment glyph: eight and sixteen records per lane, whose bands with three or more
    over-full rows walk their pairs three times through the same body"""
    gs = GlyphSet([_of_class(make, segs, {8: 2, 16: 3}[rpl], 1200 + segs)])
    jobs, shape = _place([(0, 0, 256, 256, 192, 0.125)])
    got, ref, desc = _render_both(ctx, oracle, gs, jobs, shape, fr.FR_COVERAGE_U8, 4, True)
    assert _first(desc) == f"fr::cov4_kernel<4, 32, {rpl}, 4>", desc
    _same(got, ref, desc)


def test_headline_fill_twin(ctx, oracle):
    g = _synth_with_roots(128, 129, 256, 628)
    gs = GlyphSet([g])
    s32 = float(np.float32(1.0 / 8))
    jobs, shape = _place([(0, int(np.floor(g.box.x_min * s32)) - 3, int(np.ceil((g.box.y_min + g.box.y_max) / 2 * s32)) + 40, 144, 80, s32)])
    got, ref, desc = _render_both(ctx, oracle, gs, jobs, shape, fr.FR_COVERAGE_U8, 4, True, fill=1)
    assert desc.split("; ")[0] == "fr::cov4_kernel<4, 32, 4, 4, 1> x1", desc
    _same(got, ref, desc)


# ---- toggle signs ---------------------------------------------------------------------------------------------------
def _rect(x0, y0, x1, y1, clockwise=True):
    p = [(x0, y0), (x0, y1), (x1, y1), (x1, y0)]            # clockwise in y-up units
    return p if clockwise else p[::-1]


@pytest.mark.parametrize("clockwise", [True, False], ids=["cw", "ccw"])
def test_toggle_signs(ctx, oracle, clockwise):
    """at scale 1/4 and the centre phase sample column j of a cell with min_x = 0 lies at x = j + 1/2, so a vertical edge
    at x = 16 q + 15 has J = 16 q + 15 columns on its left: sample 3 of the pixel in byte 3 of a dword of E, whose second
    difference lands in the next dword.  Rectangles with such edges, two of them overlapping in the same direction
    (winding +2 or -2 by orientation), next to a comb of 12 teeth: 24 crossings on a row."""
    rects = [_rect(15, 40, 47, 300, clockwise), _rect(31, 120, 79, 380, clockwise), _rect(95, 30, 111, 90, clockwise),
             _rect(303, 200, 559, 390, clockwise), _rect(319, 220, 543, 300, clockwise)]
    cs, _ = comb_glyph(12)
    comb = [np.asarray(c, np.int16) for c in cs]
    allp = np.concatenate(comb)
    gs = GlyphSet([_poly_glyph(rects), Glyph(Box(int(allp[:, 0].min()), int(allp[:, 1].min()), int(allp[:, 0].max()), int(allp[:, 1].max())),
                                             [Contour(c) for c in comb])])
    jobs, shape = _place([(0, 0, 100, 150, 100, 0.25), (1, 0, 101, 240, 101, 0.125)])
    wd, wref, _ = _render_both(ctx, oracle, gs, jobs, shape, fr.FR_WINDING_I16, 1, False)
    _same(wd, wref, "windings")
    assert (np.abs(wref[2:102, 3:153]) == 2).any()
    for n in (4, 2):
        got, ref, desc = _render_both(ctx, oracle, gs, jobs, shape, fr.FR_COVERAGE_U8, n, True)
        _same(got, ref, (n, desc))
        # 4 x 4: the edge at x = 15 leaves sample column 15 alone of pixel 3's four inside the first rectangle
        if n == 4:
            assert int(ref[2 + 50, 3 + 3]) == 64 and int(ref[2 + 50, 3 + 2]) == 0

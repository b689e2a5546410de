"""Candidate records (option "cand_records"): the fast kernels' set-up reads each candidate
root's record ready-made from a table that fr_glyphset_create built once per glyph, live candidates first and in record
order.  Here: the table against records rebuilt on the device (fr_selftest_cand_records), glyphs whose live count sits on
either side of every wave boundary of the set-ups, and one plan that mixes them.  Byte equality with the oracle and with
the same render under cand_records = 0, over sentinel-filled arrays."""
import numpy as np
import pytest

import font_renderer_amd as fr
import oracle_lib as O
from font_renderer_amd import render_glyph as rg
from font_renderer_amd.atlas import cell_jobs
from font_renderer_amd.glyph import Box, Contour, Glyph, GlyphSet
from font_renderer_amd.synth import stroke_glyphset, synth_glyph, synth_glyphset

pytestmark = pytest.mark.gpu
SENT = 0x5b
OMODE = {fr.FR_GRAY_DEBUG: O.GRAY_DEBUG, fr.FR_COVERAGE_U8: O.COVERAGE_U8}
CORNER, CENTER = fr.FR_SAMPLE_CORNER, fr.FR_SAMPLE_CENTER
# live counts on either side of one, two, three and four waves of 64 lanes
BOUNDARIES = (64, 65, 128, 129, 192, 193, 256)


def _glyph(contours):
    cs = [Contour(np.array(c, np.int16)) for c in contours]
    allp = np.concatenate([c.points for c in cs])
    return Glyph(Box(int(allp[:, 0].min()), int(allp[:, 1].min()), int(allp[:, 0].max()), int(allp[:, 1].max())), cs)


def _vertex_rule_live(contours):
    """the candidate roots record_prep (fr_records.hpp) keeps: a == 0: the one root unless p2y == p0y; else the far-side
    root unless t_v = b / a >= 1 and the near-side root unless t_v < 0.  An upper bound of the live count (a kept
    candidate whose cut is empty is not live): the device decides, this only steers the search below."""
    n = 0
    for c in contours:
        y = np.asarray(c, np.int64)[:, 1]
        if len(y) < 3:
            continue
        p0, p1, p2 = y[0:-1:2], y[1::2], y[2::2]
        a, b = p0 - 2 * p1 + p2, p0 - p1
        tv_ge1 = np.where(a > 0, b >= a, b <= a)
        tv_lt0 = b * a < 0
        for root in (0, 1):
            far = (a > 0) if root == 0 else (a < 0)
            n += int(np.where(a == 0, (p2 != p0) if root == 0 else False, np.where(far, ~tv_ge1, ~tv_lt0)).sum())
    return n


def _selftest(ctx, gs):
    dgs = fr.DeviceGlyphSet(ctx, gs)
    try:
        live, bad, first, per_glyph = dgs.selftest_cand_records()
    finally:
        dgs.close()
    assert bad == 0, (bad, "first (glyph, slot):", first)
    assert live == int(per_glyph.sum())
    assert (per_glyph <= 2 * gs.segments_per_glyph()).all()
    return per_glyph


def test_selftest_ascii_fixture(ctx, ascii_set):
    live = _selftest(ctx, ascii_set.gs)
    assert live.sum() > 0


@pytest.mark.parametrize("segments", [16, 32, 64, 128, 256, "stroke128"])
def test_selftest_synthetic_glyphs(ctx, segments):
    gs = stroke_glyphset(8, 128) if segments == "stroke128" else synth_glyphset(8, segments)
    live = _selftest(ctx, gs)
    assert (live > 0).all()
    if segments == 256:
        assert (live > 256).all()                  # (the set-up's second pass has live candidates)


def _hand_made():
    m, M = -32768, 32767
    return [
        ("horizontal lines only", [[(0, 5), (4, 5), (8, 5), (12, 5), (16, 5)], [(0, -3), (-5, -3), (-10, -3)]], 0),
        ("one segment", [[(0, 0), (4, 12), (20, 8)]], None),
        ("one straight segment", [[(0, 0), (2, 5), (4, 10)]], 1),
        ("lines only", [[(0, 8), (4, 12), (8, 16), (12, 12), (16, 8), (12, 4), (8, 0), (4, 4), (0, 8)]], 4),
        ("vertex at t = 0", [[(0, 0), (4, 0), (8, 8)]], None),
        ("vertex at t = 1", [[(0, 8), (4, 0), (8, 0)]], None),
        ("vertex at t = 0, opening down", [[(0, 0), (4, 0), (8, -8)]], None),
        ("i16 extremes", [[(m, m), (m, 0), (m, M), (0, M), (M, M), (M, 1), (M, m), (0, m), (m, m)],
                          [(m, 0), (-5, M), (M, 3), (7, m), (m, 0)],
                          [(-3, m), (M, -32767), (-2, M), (m, 32766), (-3, m)]], None),
    ]


def test_selftest_hand_made_glyphs(ctx):
    cases = _hand_made()
    gs = GlyphSet([_glyph(c) for _, c, _ in cases])
    live = _selftest(ctx, gs)
    for g, (name, contours, want) in enumerate(cases):
        assert live[g] <= _vertex_rule_live(contours), name
        if want is not None:
            assert live[g] == want, (name, int(live[g]), want)
    assert live[1] > 0 and live[4] > 0 and live[5] > 0 and live[7] > 0


def _variants(target):
    """synthetic glyphs with segments dropped from the end of their last contour, whose vertex-rule count is near `target`"""
    out = []
    for idx in range(8):
        contours, _ = synth_glyph(idx, int(np.ceil(target / 1.2)) + 4)
        contours = [c.copy() for c in contours]
        while _vertex_rule_live(contours) >= target - 2 and len(contours[-1]) >= 5:
            if _vertex_rule_live(contours) <= target + 2:
                out.append([c.copy() for c in contours])
            contours[-1] = contours[-1][:-2]
    return out


@pytest.fixture(scope="module")
def boundary_set(ctx):
    """one glyph per live count of BOUNDARIES (the count as fr_selftest_cand_records reports it), a 256-segment glyph with
    more than 256 live candidates, and a 20-segment glyph for the one-wave set-up -> (GlyphSet, live counts)"""
    chosen = []
    for target in BOUNDARIES:
        cand = _variants(target)
        assert cand, target
        live = _selftest(ctx, GlyphSet([_glyph(c) for c in cand]))
        hit = np.flatnonzero(live == target)
        assert len(hit), (target, sorted(set(live.tolist())))
        chosen.append(cand[int(hit[0])])
    chosen.append(synth_glyph(0, 256)[0])
    chosen.append(synth_glyph(1, 20)[0])
    gs = GlyphSet([_glyph(c) for c in chosen])
    live = _selftest(ctx, gs)
    assert tuple(live[:len(BOUNDARIES)].tolist()) == BOUNDARIES, live
    assert live[len(BOUNDARIES)] > 256 and gs.segments_per_glyph()[len(BOUNDARIES)] == 256
    return gs, live


def _render(ctx, dgs, jobs, mode, shape, n, phase):
    out = np.full(shape, SENT, np.uint8)
    return rg.render_batch(dgs, jobs, mode, out, n, phase)


def _oracle(oracle, gs, jobs, mode, shape, n, phase):
    out = np.full(shape, SENT, np.uint8)
    return oracle.render_batch(gs, jobs, OMODE[mode], out, n, phase == CENTER, 16)


def _both_ways(ctx, dgs, jobs, mode, shape, n, phase):
    """the render with cand_records = 1 and = 0 (byte-equal, from the same launches) -> the first, the plan's description"""
    got = {}
    try:
        for cand in (1, 0):
            ctx.set_option("cand_records", cand)
            plan = fr.Plan(dgs, jobs, mode, n, phase)
            desc, st = plan.describe(), plan.stats()
            plan.close()
            got[cand] = (_render(ctx, dgs, jobs, mode, shape, n, phase), desc, st)
    finally:
        ctx.set_option("cand_records", 1)
    assert got[1][1] == got[0][1], (got[1][1], got[0][1])
    assert got[1][2]["jobs_general"] == 0, got[1][1]
    assert np.array_equal(got[1][0], got[0][0]), (got[1][1], np.argwhere(got[1][0] != got[0][0])[:4].tolist())
    return got[1][0], got[1][1]


@pytest.mark.parametrize("mode,n,phase,kernel", [(fr.FR_COVERAGE_U8, 4, CENTER, "cov4_kernel"), (fr.FR_GRAY_DEBUG, 1, CORNER, "win1_kernel")])
@pytest.mark.parametrize("which", list(range(len(BOUNDARIES) + 2)))
def test_setup_boundaries(ctx, oracle, boundary_set, which, mode, n, phase, kernel):
    """each boundary glyph alone in a 64 x 64 cell: the oracle's bytes, and the bytes of cand_records = 0"""
    gs, _ = boundary_set
    jobs = cell_jobs(gs, 64, 64, 2048, 1, first_glyph=which, n_glyphs=1)
    dgs = fr.DeviceGlyphSet(ctx, gs)
    try:
        got, desc = _both_ways(ctx, dgs, jobs, mode, (65, 64), n, phase)
    finally:
        dgs.close()
    assert kernel in desc, desc
    want = _oracle(oracle, gs, jobs, mode, (65, 64), n, phase)
    assert np.array_equal(got, want), (which, desc, np.argwhere(got != want)[:4].tolist())
    assert (got[64] == SENT).all() and (want[:64] != SENT).any() and (want[:64] != want[0, 0]).any()


@pytest.mark.parametrize("mode,n,phase", [(fr.FR_COVERAGE_U8, 4, CENTER), (fr.FR_GRAY_DEBUG, 1, CORNER)])
def test_one_plan_mixing_the_boundary_glyphs(ctx, oracle, boundary_set, mode, n, phase):
    """all of them in one plan, at a power-of-two scale (64 px per em of 2 048) in 64 x 64 cells and at a scale that is none
    (45 px per em) in ragged 47 x 45 cells"""
    gs, _ = boundary_set
    a = cell_jobs(gs, 64, 64, 2048, len(gs))
    b = cell_jobs(gs, 64, 45, 2048, len(gs))
    b["w"], b["h"] = 47, 45
    b["out_y"] += 64
    assert float(a["scale"][0]) == 2.0 ** -5 and np.frexp(float(b["scale"][0]))[0] != 0.5
    jobs = np.concatenate([a, b])
    shape = (64 + 45 + 1, 64 * len(gs))
    dgs = fr.DeviceGlyphSet(ctx, gs)
    try:
        got, desc = _both_ways(ctx, dgs, jobs, mode, shape, n, phase)
    finally:
        dgs.close()
    want = _oracle(oracle, gs, jobs, mode, shape, n, phase)
    assert np.array_equal(got, want), (desc, np.argwhere(got != want)[:4].tolist())
    assert (got[-1] == SENT).all() and (got[64:, 47:64] == SENT).all() and (want[:64] != SENT).any()

"""The block-glyph cases (tests/text_block_cases.py) on the CPU: the generators' invariants, the exact reference against
the float twins sample for sample on every case the GPU tests render, and the colour cases against the definitions and
against what their enumerations claim to reach.  No GPU."""
from fractions import Fraction as Fr

import numpy as np
import pytest

import fill_rule_ref as FR
import oracle_lib as O
import ref_numpy
import text_block_cases as B
import text_twin as tw

F = np.float32


def _f32(vals):
    out = np.array([float(v) for v in vals], F)
    assert all(Fr(float(o)) == Fr(v) for o, v in zip(out, vals))              # the exact values ARE binary32 values
    return out


# ---- 1. generator invariants ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 4])
def test_cover_lights_exactly_k_samples(n):
    """cover(k, W, n) covers exactly k of each pixel's n^2 centre-phase samples, for every k, under the exact rule, the
    consistent twin and the reference's rule alike; no sample lies on an edge; every inside sample is in the cell"""
    s = Fr(1, 8)
    for W in (1, 3, 86):
        for k in range(1, n * n + 1):
            g = B.cover(k, W, n)
            assert g.box == (0, 0, 8 * W, 8)
            mn_x, mx_y, w, h = B.job_cell(g.box, s)
            assert (mn_x, mx_y, w, h) == (0, 1, W + 1, 2)
            ts_, cys = B.job_axes(mn_x, mx_y, w, h, s, n, True)
            wd = B.windings(g, ts_, cys)
            assert set(np.unique(wd)) <= {0, 1} and B.on_edge_samples(g, ts_, cys) == 0
            cnt = wd.reshape(h, n, w, n).sum(axis=(1, 3))
            want = np.zeros((h, w), int)
            want[0, :W] = k
            assert np.array_equal(cnt, want), (n, k, W)
            if W < 86 or k in (1, n * n - 1, n * n):
                gs = B.glyph_set([g])
                cx, cy = _f32(ts_), _f32(cys)
                assert np.array_equal(FR.winding_fill(gs.points_xy, gs.contour_start, cx[None, :], cy[:, None]), wd)
                assert np.array_equal(ref_numpy.winding_at(gs.points_xy, gs.contour_start, cx[None, :], cy[:, None]), wd)
    assert B.cover(0, 5, n) is None


def test_the_two_rules_on_a_square():
    """on the square [0, 16]^2 the consistent rule is inside exactly for 0 <= cy < 16, 0 < cx <= 16; the reference's rule
    differs on the rows cy = 0 and cy = 16 only"""
    sq = B.edge_glyphs()[0]
    gs = B.glyph_set([sq])
    grid = [Fr(v, 2) for v in range(-4, 37)]
    for y in grid:
        for x in grid:
            assert B.inside_exact(sq, x, y) == (0 <= y < 16 and 0 < x <= 16), (x, y)
    c = _f32(grid)
    ref = ref_numpy.winding_at(gs.points_xy, gs.contour_start, c[None, :], c[:, None]) != 0
    fill = FR.winding_fill(gs.points_xy, gs.contour_start, c[None, :], c[:, None]) != 0
    differ = np.nonzero((ref != fill).any(axis=1))[0]
    assert sorted(float(c[r]) for r in differ) == [0.0, 16.0]


def test_edge_glyphs_are_what_they_claim():
    gl = {g.name: g for g in B.edge_glyphs()}
    assert len(gl) == 12
    for g in gl.values():                                      # even coordinates, inside +-64
        assert all(not (x | y) & 1 and abs(x) <= 64 and abs(y) <= 64 for c in g.contours for x, y in c), g.name

    def quad(name):
        (p0, p1, p2), = [s for s in gl[name].segments() if s[0][1] - 2 * s[1][1] + s[2][1] != 0]
        a, b = p0[1] - 2 * p1[1] + p2[1], p0[1] - p1[1]
        return a, Fr(b, a), p0[1] - Fr(b * b, a)
    assert quad("bump") == (-64, Fr(1, 2), 16)                  # the vertex is the high end
    assert quad("bowl") == (64, Fr(1, 2), 0)                    # the vertex is the low end
    assert quad("quarter")[1] == 1 and quad("bulge")[1] == Fr(3, 2) and quad("sweep")[1] == 0
    assert len(B.pieces(gl["bump"])) == 2 and len(B.pieces(gl["sweep"])) == 2     # (sweep: its near side is a point)
    # hand counts: the ring's hole, the overlap's winding 2, the notch's extremum crossed twice, the bump's tangent row
    assert B.winding_exact(gl["ring"], 0, 0) == 0 and B.winding_exact(gl["ring"], 24, 0) == 1
    assert B.winding_exact(gl["two"], 24, 24) == 2 and B.winding_exact(gl["two"], 8, 8) == 1
    assert B.winding_exact(gl["notch"], 16, 16) == 1 and B.winding_exact(gl["notch"], 16, 17) == 0
    assert B.winding_exact(gl["notch"], 8, 24) == 1 and B.winding_exact(gl["notch"], 28, 24) == 1 and B.winding_exact(gl["notch"], 16, 24) == 0
    assert B.winding_exact(gl["bump"], 16, 16) == 0 and B.winding_exact(gl["bump"], 16, 15) == 1
    assert B.winding_exact(gl["bowl"], 16, 0) == 1 and B.winding_exact(gl["bowl"], 16, 1) == 0 and B.winding_exact(gl["bowl"], 4, 0) == 1
    assert B.winding_exact(gl["diamond"], 0, 16) == 0 and B.winding_exact(gl["diamond"], 0, -16) == 0
    assert B.winding_exact(gl["diamond"], 16, 0) == 1 and B.winding_exact(gl["diamond"], -16, 0) == 0
    for name in ("square", "square5", "stairs"):
        assert B.winding_exact(gl[name], 4, 0) == 1 and B.winding_exact(gl[name], 4, 32 if name == "stairs" else 16) == 0
    # every curved outline keeps the margin condition on at least eight grids, among them 16 samples per pixel
    for name in B.CURVED:
        ok = [(s, n, c) for s, n, c in B.GRIDS if B.grid_ok(gl[name], s, n, c)]
        assert len(ok) >= 8 and any(n == 4 for _, n, _ in ok), (name, ok)
    # scale 1/4, corner phase, n = 4: a sample row on every integer height of the bump, its vertex row included
    _, cys = B.job_axes(*B.job_cell(gl["bump"].box, Fr(1, 4)), Fr(1, 4), 4, False)
    assert set(range(0, 33)) <= set(cys) and B.grid_ok(gl["bump"], Fr(1, 4), 4, False)


# ---- 2. the exact reference and the twins, sample for sample ---------------------------------------------------------------
def _same_samples(glyphs, places, runs, n, center, ex):
    gs = B.glyph_set(glyphs)
    lit = 0
    for run in runs:
        exact = B.run_hits(glyphs, places, run, n, center)
        twin = tw.coverage_samples("ex" if ex else "plain", gs, places, run, n, center, True)
        assert exact.shape == twin.shape and np.array_equal(exact, twin), (n, center, ex, int(run["first"]))
        lit += int(exact.sum())
    assert B.cells_hold_the_glyphs(glyphs, places, runs, n, center)
    return lit


@pytest.mark.parametrize("ex", [False, True])
def test_exact_reference_equals_the_twin_on_the_edge_rows(ex):
    for s, n, center in B.GRIDS:
        glyphs, places, runs, _ = B.edge_row_case(s, n, center, ex)
        assert len(runs) >= 8 and int(runs[-1]["count"]) == len(runs) - 1       # the last run overlaps all the glyphs
        assert _same_samples(glyphs, places, runs, n, center, ex) > 0


@pytest.mark.parametrize("ex", [False, True])
def test_exact_reference_equals_the_twin_on_pen_fractions_and_tiles(ex):
    cases = B.pen_fraction_cases(ex)
    bump_pens = set()
    for (n, center), (glyphs, places, runs, _) in cases.items():
        sq = places[places["glyph"] == 0]
        assert set((sq["pen_x64"] % 64).tolist()) == set(range(64))
        if ex:
            assert set((sq["pen_y64"] % 64).tolist()) == set(range(64))
            bump_pens |= {(int(p["pen_x64"]) % 64, int(p["pen_y64"]) % 64) for p in places[places["glyph"] == 1]}
        else:
            bump_pens |= {(int(p["pen_x64"]) % 64, 0) for p in places[places["glyph"] == 1]}
        _same_samples(glyphs, places, runs, n, center, ex)
    assert {fx for fx, fy in bump_pens if fy == 0} == set(range(64))
    assert not ex or {fy for _, fy in bump_pens} == set(range(64))
    # fx64 = 0, 8, 16, ...: samples exactly on the square's vertical edges, at one phase or the other
    # (the samples are 2 units apart, a pen fraction of f / 64 pixel moves them by f / 8 unit)
    for center, fractions in ((False, (0, 16, 32, 48)), (True, (8, 24, 40, 56))):
        glyphs, places, runs, _ = cases[(4, center)]
        for f in fractions:
            k = next(i for i, p in enumerate(places) if p["glyph"] == 0 and p["pen_x64"] % 64 == f)
            _, px, py, s, _ = B.place_of(places[k], runs[k])
            axes = B.place_axes(0, int(runs[k]["w"]), 0, int(runs[k]["h"]), s, px, py, 4, center)
            assert B.on_edge_samples(glyphs[0], *axes) > 0, f
    for n, center in B.PHASES:
        glyphs, places, runs, _ = B.tile_case(ex)
        _same_samples(glyphs, places, runs, n, center, ex)


def test_tile_case_is_what_it_claims():
    glyphs, places, runs, _ = B.tile_case(True)
    gs = B.glyph_set(glyphs)
    lists = {}
    for k in range(int(runs[0]["count"])):
        _, px, py, s, sl = B.place_of(places[k], runs[0])
        c0, r0, cw, ch = B.place_cell(glyphs[int(places[k]["glyph"])].box, s, sl, px, py)
        for ty in range(max(r0, 0) // 16, (min(r0 + ch, 44) - 1) // 16 + 1):
            for tx in range(max(c0, 0) // 64, (min(c0 + cw, 200) - 1) // 64 + 1):
                lists.setdefault((ty, tx), []).append(k)
    assert len(lists[(2, 0)]) >= 40 and len(lists) >= 10        # one tile lists 40 placements; 10 of the 12 tiles are met
    assert tw.met_tiles("ex", gs, places, runs[:1]) == {(0, ty, tx) for ty, tx in lists}
    assert int(runs[1]["w"]) < 64 and int(runs[1]["out_x"]) % 4 != 0
    # the pen at 55 + 32/64 has a cell of 10 columns: 55 .. 63 and the extra column 64, in the next tile
    assert 4 in lists[(1, 0)] and 4 in lists[(1, 1)] and 5 in lists[(2, 1)] and 5 in lists[(2, 2)]


@pytest.mark.parametrize("n,center", B.PHASES)
def test_exact_reference_equals_the_twin_on_scales_and_slants(n, center):
    glyphs, places, runs, _ = B.slant_case(n, center)
    assert set(places["slant"].tolist()) == {float(k) for k in B.SLANTS}
    assert set(places["scale"].tolist()) == {0.0} | {float(s) for s in B.SCALES}
    assert len({int(p["pen_y64"]) % 64 for p in places}) > 32 and len(set(places["glyph"].tolist())) == 12
    assert _same_samples(glyphs, places, runs, n, center, True) > 0
    # a slanted vertical edge passes exactly through sample points
    on_edge = 0
    for p, r in zip(places, runs):
        gi, px, py, s, k = B.place_of(p, r)
        if k != 0 and glyphs[gi].name == "square":
            on_edge += B.on_edge_samples(glyphs[gi], *B.place_axes(0, int(r["w"]), 0, int(r["h"]), s, px, py, n, center), k)
    assert on_edge > 0


def test_reference_rule_twin_equals_the_oracle_on_the_job_cells(oracle):
    """flags = 0 on the same raster cells: ref_numpy.winding_at == the C oracle, windings and coverage"""
    for s, n, center in B.GRIDS:
        glyphs, jobs, shape = B.job_case(s, n, center)
        gs = B.glyph_set(glyphs)
        assert len(jobs) >= 7
        for j in jobs:
            pts, cs = tw.glyph_arrays(gs, int(j["glyph"]))
            cell = (int(j["min_x"]), int(j["max_y"]), int(j["w"]), int(j["h"]), j["scale"])
            cx, cy = FR.sample_axes(*cell, n, center)
            wd = ref_numpy.winding_at(pts, cs, cx[None, :], cy[:, None])
            g = glyphs[int(j["glyph"])].glyph()
            if n == 1:
                assert np.array_equal(wd, oracle.render_cell(g, *cell, O.WINDING_I16, 1, center)), (float(s), center)
            assert np.array_equal(FR.to_mode(wd.astype(np.int32), FR.COVERAGE_U8, n),
                                  oracle.render_cell(g, *cell, O.COVERAGE_U8, n, center)), (float(s), n, center)
        # and the consistent rule: exact == twin on the same cells
        exact = B.job_windings(glyphs, jobs, shape, n, center)
        for j in jobs:
            pts, cs = tw.glyph_arrays(gs, int(j["glyph"]))
            cx, cy = FR.sample_axes(int(j["min_x"]), int(j["max_y"]), int(j["w"]), int(j["h"]), j["scale"], n, center)
            oy, ox = int(j["out_y"]) * n, int(j["out_x"]) * n
            assert np.array_equal(FR.winding_fill(pts, cs, cx[None, :], cy[:, None]), exact[oy:oy + len(cy), ox:ox + len(cx)])


# ---- 3. colour cases -------------------------------------------------------------------------------------------------------
def test_colour_formulas_are_the_definitions():
    """blend_rgba / blend_srgb / mix_* against the definition twins, and the identities the cases lean on"""
    rng = np.random.default_rng(5)
    dst = rng.integers(0, 256, (500, 4)).astype(np.int64)
    for col in [(0, 255, 17, 0), (200, 3, 99, 255), (5, 6, 7, 128), (255, 255, 255, 1)]:
        for blend, fn in ((tw.blend, B.blend_rgba), (tw.srgb_blend, B.blend_srgb)):
            assert np.array_equal(blend(dst, col)[:, :3], fn(np.array(col[:3]), dst[:, :3], col[3]))
    v = np.arange(256)
    assert np.array_equal(tw.E[tw.D[v]], v)                     # an untouched sRGB sample resolves to itself
    for n in (1, 2, 4):
        smp = rng.integers(0, 256, (n, 7 * n, 4)).astype(np.int64)
        parts = [(1, smp.reshape(1, n, 7, n, 4)[0, a, :, b]) for a in range(n) for b in range(n)]
        assert np.array_equal(tw.resolve(smp, n)[0], B.mix_rgba(parts, n))
        assert np.array_equal(tw.srgb_resolve(smp, n)[0, :, :3], B.mix_srgb([(k, p[:, :3]) for k, p in parts], n))


def _twin_rows(case, n, srgb, load, count, h):
    """the definition twins on the run cut down to its first `count` placements and `h` rows"""
    gs = B.glyph_set(case.glyphs)
    r = case.runs[0]
    run = np.array([(0, count, int(r["w"]), h, 1, 1, r["scale"])], B.rg.RUN_DTYPE)
    ex = "pen_y64" in case.places.dtype.names
    out = case.start[:h + 2].copy()
    got = tw.rgba_render_runs("ex" if ex else "plain", gs, case.places, case.rgba, run, case.clears, out, n, True, False, srgb, False, load)
    return got[1:h + 1], case.want[1:h + 1]


@pytest.mark.parametrize("n,ex,srgb", [(4, False, False), (2, True, True), (1, False, True), (4, True, True)])
def test_colour_cases_equal_the_definition_twins_on_their_first_rows(n, ex, srgb):
    for case, count, h in [(B.blend_load_case(n, ex, srgb), 16, 2), (B.two_layer_case(n, ex, srgb), 64, 2),
                           (B.opaque_load_case(n, ex, srgb), 2 * n * n, 2)]:
        got, want = _twin_rows(case, n, srgb, True, count, h)
        assert np.array_equal(got, want)
    for load in (True, False):
        case = B.opaque_overlap_case(n, ex, srgb, load)
        got, want = _twin_rows(case, n, srgb, load, len(case.places), int(case.runs[0]["h"]))
        assert np.array_equal(got, want), load
    for build in (B.blend_clear_case, B.opaque_clear_case):
        case = build(n, ex, srgb)
        gs = B.glyph_set(case.glyphs)
        which = [0, 1, 100, 255]
        out = case.start.copy()
        tw.rgba_render_runs("ex" if ex else "plain", gs, case.places, case.rgba, case.runs, case.clears, out, n, True, False, srgb, False, False, which)
        for r in which:
            assert np.array_equal(out[1 + r], case.want[1 + r]), (build.__name__, r)


def test_the_enumerations_reach_what_they_claim():
    # every (C, c, A) triple, in every colour channel position the blend kernels have
    case = B.blend_load_case(4, False, True)
    C, c, A = (np.broadcast_to(v, case.c.shape).reshape(-1).astype(np.int64) for v in (case.C, case.c, case.A))
    seen = np.zeros(1 << 24, bool)
    seen[(C << 16) | (c << 8) | A] = True
    assert seen.all()
    L = (tw.D[C] * A + tw.D[c] * (255 - A) + 127) // 255
    assert len(np.unique(L)) >= 65502 and len(np.unique(L >> 4)) == 4096      # the linear values, the entries of SRGB_K
    assert (case.want[1:-1, 1:-1, 3] == case.A[..., 0]).all()
    bg = B.blend_load_case(4, False, False, bgra=True)
    assert not np.array_equal(bg.want, B.blend_load_case(4, False, False).want)
    # the clear-colour family: every pair out of C, c and A
    case = B.blend_clear_case(4, False, False)
    C, c, A = (np.broadcast_to(v, case.c.shape)[..., 0].reshape(-1) for v in (case.C, case.c, case.A))
    for a, b in ((C, c), (C, A), (c, A)):
        assert len(np.unique(a * 256 + b)) == 65536
    # the opaque resolve: every (k, C, c), and the linear values it reaches with 16 samples
    for n in (1, 2, 4):
        case = B.opaque_load_case(n, False, True)
        k, C, c = (np.broadcast_to(v, case.c.shape).reshape(-1) for v in (case.k, case.C, case.c))
        assert len(np.unique((k << 16) | (C << 8) | c)) == (n * n + 1) * 65536
        if n == 4:
            L = (k * tw.D[C] + (16 - k) * tw.D[c] + 8) >> 4
            assert len(np.unique(L)) >= 60846 and len(np.unique(L >> 4)) >= 4080
        case = B.opaque_clear_case(n, False, False)
        assert len(np.unique(case.C[..., 0] * 256 + case.c[..., 0])) == 65536
        assert set(np.unique(case.k)) == set(range(n * n + 1))
    case = B.two_layer_case(4, False, True)
    assert len(set(zip(case.A1.tolist(), case.A2.tolist()))) == 4096 and {0, 255} <= set(case.A1.tolist())

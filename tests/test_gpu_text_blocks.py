"""Block glyphs on the GPU (tests/text_block_cases.py): sample rows through every piece end, every pen fraction, dyadic
scales and slants, tile borders, and the same outlines as fr_job cells.  Under FR_FILL_CONSISTENT the expected image is
exact integer geometry (no float twin in the loop: one ulp, one sample or one row wrong fails); under flags = 0 the
kernels must miscount exactly as the reference's rule does, so there the twin (text plans) or the C oracle (fr_job cells)
is the expectation.  Sentinel-filled buffers, runs at odd offsets, the whole array compared with np.array_equal."""
from contextlib import closing

import numpy as np
import pytest

import font_renderer_amd as fr
import text_block_cases as B
import text_gpu as G
from font_renderer_amd import render_glyph as rg
from text_gpu import FILL

pytestmark = pytest.mark.gpu
SENT = B.SENT


def _check_text(ctx, glyphs, places, runs, shape, n, center, tag):
    """both rules of one text case: FR_FILL_CONSISTENT == the exact geometry, flags = 0 == the twin of the reference's rule"""
    ex = "pen_y64" in places.dtype.names
    gs = B.glyph_set(glyphs)
    kernel = "fr::text_%skernel<%d, %%d>" % ("place_" if ex else "", n)
    assert runs["out_x"].min() % 2 == 1 and runs["out_y"].min() % 2 == 1
    with closing(fr.DeviceGlyphSet(ctx, gs)) as dgs:
        info = {}
        got = G.render_gray(ctx, dgs, places, runs, shape, fr.FR_COVERAGE_U8, n, center, FILL, sent=SENT, info=info)
        assert kernel % 1 in info["describe"], (tag, info)
        want = B.render_runs(glyphs, places, runs, np.full(shape, SENT, np.uint8), n, center)
        assert np.array_equal(got, want), (tag, "fill", np.argwhere(got != want)[:8].tolist())
        assert (want != SENT).any() and (want == 255).any()
        got = G.render_gray(ctx, dgs, places, runs, shape, fr.FR_COVERAGE_U8, n, center, 0, sent=SENT, info=info)
        assert kernel % 0 in info["describe"], (tag, info)
        twin = G.twin_gray("ex" if ex else "plain", gs, places, runs, shape, n, center, False, sent=SENT)
        assert np.array_equal(got, twin), (tag, "reference rule", np.argwhere(got != twin)[:8].tolist())
        if n == 1:                                             # FR_MASK_NONZERO is the same kernel instance and the same bytes
            mask = G.render_gray(ctx, dgs, places, runs, shape, fr.FR_MASK_NONZERO, 1, center, FILL, sent=SENT, info=info)
            assert kernel % 1 in info["describe"] and np.array_equal(mask, want), tag
        return want, twin


@pytest.mark.parametrize("ex", [False, True], ids=["place", "place_ex"])
def test_rows_through_every_piece_end(ctx, ex):
    """every edge glyph alone and all of them overlapping in one run, on every grid of B.GRIDS: at scale 1/4, corner
    phase, n = 4 a sample row sits on every integer height, so on every vertex, extremum and horizontal edge"""
    differ = 0
    for s, n, center in B.GRIDS:
        glyphs, places, runs, shape = B.edge_row_case(s, n, center, ex)
        want, twin = _check_text(ctx, glyphs, places, runs, shape, n, center, (float(s), n, center))
        differ += int((want != twin).sum())
    assert differ > 0                                          # the reference's rule does miscount some of these rows


@pytest.mark.parametrize("ex", [False, True], ids=["place", "place_ex"])
def test_every_pen_fraction(ctx, ex):
    """fx64 = 0 .. 63 (and fy64 = 0 .. 63 under fr_glyph_place_ex) against the square and the bump"""
    for (n, center), (glyphs, places, runs, shape) in B.pen_fraction_cases(ex).items():
        _check_text(ctx, glyphs, places, runs, shape, n, center, ("pen", n, center))


@pytest.mark.parametrize("n,center", B.PHASES)
def test_scales_slants_and_baselines(ctx, n, center):
    """fr_glyph_place_ex: every scale of {1/8 .. 2} with every slant of {0, +-1/2, +-1, 2, 4}, pen fractions in both
    axes; the expected sample is inside_exact at (t - k cy, cy)"""
    glyphs, places, runs, shape = B.slant_case(n, center)
    _check_text(ctx, glyphs, places, runs, shape, n, center, ("slant", n, center))


@pytest.mark.parametrize("ex", [False, True], ids=["place", "place_ex"])
def test_tile_borders(ctx, ex):
    """block edges on the tile borders, a cell whose extra column is the next tile's first, 40 placements in one tile's
    list, and a run narrower than a tile at an unaligned out_x"""
    glyphs, places, runs, shape = B.tile_case(ex)
    for n, center in B.PHASES:
        _check_text(ctx, glyphs, places, runs, shape, n, center, ("tiles", n, center))


# ---- the stand-alone records elsewhere: the same outlines as fr_job cells ---------------------------------------------------
def _exact_jobs(glyphs, jobs, shape, n, center, mode):
    wd = B.job_windings(glyphs, jobs, shape, n, center)
    if mode == fr.FR_WINDING_I16:
        return np.where(wd == -32768, SENT, wd).astype(np.int16)
    out = np.full(shape, SENT, np.uint8)
    for j in jobs:
        oy, ox, h, w = int(j["out_y"]), int(j["out_x"]), int(j["h"]), int(j["w"])
        out[oy:oy + h, ox:ox + w] = B.coverage_bytes(wd[oy * n:(oy + h) * n, ox * n:(ox + w) * n] != 0, n)
    return out


def _render_jobs(ctx, dgs, jobs, mode, shape, n, center, flags):
    with closing(fr.Plan(dgs, jobs, mode, n, G.phase(center), flags)) as plan:
        desc = plan.describe()
    out = np.full(shape, SENT, np.int16 if mode == fr.FR_WINDING_I16 else np.uint8)
    rg.render_batch(dgs, jobs, mode, out, n, G.phase(center), flags)
    return out, desc


FAST = {4: "fr::cov4_kernel<", 2: "fr::cov4_kernel<", 1: "fr::win1_kernel<"}
GENERAL = {4: "fr::render_kernel<", 2: "fr::render_kernel<", 1: "fr::render_kernel<"}


@pytest.mark.parametrize("options,kernels", [((), FAST), ((("cov4", 0, 1),), GENERAL), ((("cov4", 0, 1), ("fuse_prepare", 0, 1)), GENERAL)],
                         ids=["fast", "general", "prepared"])
def test_job_cells(ctx, oracle, options, kernels):
    """the edge glyphs as fr_job cells on every grid: cov4_kernel (n = 4, 2), win1_kernel (n = 1, also the signed winding),
    render_kernel on records it builds itself (cov4 = 0) and on the stand-alone records of prepare_kernel /
    prepare_fill_kernel, the ones text plans walk (cov4 = 0, fuse_prepare = 0).  FR_FILL_CONSISTENT == the exact geometry;
    flags = 0 == the C oracle byte for byte."""
    import oracle_lib as O
    try:
        for key, value, _ in options:
            ctx.set_option(key, value)
        for s, n, center in B.GRIDS:
            glyphs, jobs, shape = B.job_case(s, n, center)
            gs = B.glyph_set(glyphs)
            with closing(fr.DeviceGlyphSet(ctx, gs)) as dgs:
                modes = [(fr.FR_COVERAGE_U8, O.COVERAGE_U8)] + ([(fr.FR_WINDING_I16, O.WINDING_I16)] if n == 1 else [])
                for mode, omode in modes:
                    got, desc = _render_jobs(ctx, dgs, jobs, mode, shape, n, center, FILL)
                    assert kernels[n] in desc, (options, n, desc)
                    want = _exact_jobs(glyphs, jobs, shape, n, center, mode)
                    assert np.array_equal(got, want), (options, float(s), n, center, mode, desc, np.argwhere(got != want)[:8].tolist())
                    got, desc = _render_jobs(ctx, dgs, jobs, mode, shape, n, center, 0)
                    ref = np.full(shape, SENT, got.dtype)
                    oracle.render_batch(gs, jobs, omode, ref, n, center)
                    assert np.array_equal(got, ref), (options, float(s), n, center, mode, desc)
    finally:
        for key, _, default in options:
            ctx.set_option(key, default)

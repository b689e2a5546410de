"""FR_FILL_CONSISTENT on the GPU: every kernel path a plan can take, against the CPU twin (tests/fill_rule_ref.py) or,
for wide coverage, the fast kernels against the general one.  Sentinel-filled outputs: bytes outside the jobs stay."""
import ctypes as C

import numpy as np
import pytest

import fill_rule_ref as FR
import font_renderer_amd as fr
from fixtures import load_font
from font_renderer_amd import _lib as L
from font_renderer_amd import render_glyph as rg
from font_renderer_amd.atlas import atlas_shape, cell_jobs
from font_renderer_amd.glyph import Box, Contour, Glyph, GlyphSet
from font_renderer_amd.synth import comb_glyph, synth_glyphset

pytestmark = pytest.mark.gpu
FILL = fr.FR_FILL_CONSISTENT
SENT = 0x5b


def _phase(center):
    return fr.FR_SAMPLE_CENTER if center else fr.FR_SAMPLE_CORNER


def _gpu(ctx, gs, jobs, mode, shape, n=1, center=False, flags=FILL, dgs=None, want=()):
    own = dgs is None
    dgs = dgs or fr.DeviceGlyphSet(ctx, gs)
    plan = fr.Plan(dgs, jobs, mode, n, _phase(center), flags)
    desc = plan.describe()
    plan.close()
    for w in want:
        assert w in desc, (w, desc)
    out = np.full(shape, SENT, np.int16 if mode == fr.FR_WINDING_I16 else np.uint8)
    rg.render_batch(dgs, jobs, mode, out, n, _phase(center), flags)
    if own:
        dgs.close()
    return out, desc


def _twin(gs, jobs, mode, shape, n=1, center=False):
    out = np.full(shape, SENT, np.int16 if mode == fr.FR_WINDING_I16 else np.uint8)
    return FR.render_batch(gs, jobs, mode, out, n, center)


def _twin_rows(gs, job, mode, rows, n=1, center=False):
    """the twin on a subset of a job's pixel rows (one-row cells at max_y - r: the same sample points)"""
    g = int(job["glyph"])
    c0, c1 = int(gs.glyph_start[g]), int(gs.glyph_start[g + 1])
    p0 = int(gs.contour_start[c0])
    pts, cs = gs.points_xy[p0:int(gs.contour_start[c1])], gs.contour_start[c0:c1 + 1] - np.uint32(p0)
    return np.concatenate([FR.render_cell(pts, cs, int(job["min_x"]), int(job["max_y"]) - int(r), int(job["w"]), 1,
                                          job["scale"], mode, n, center) for r in rows])


def _job_view(img, job):
    oy, ox = int(job["out_y"]), int(job["out_x"])
    return img[oy:oy + int(job["h"]), ox:ox + int(job["w"])]


@pytest.mark.parametrize("mode", [fr.FR_WINDING_I16, fr.FR_GRAY_DEBUG, fr.FR_MASK_NONZERO, fr.FR_COVERAGE_U8])
def test_ascii_atlas_n1_modes(ctx, ascii_set, mode):
    """95 glyphs in 128 x 128 cells at size 100 (win1_kernel), corner samples: == the twin, sentinels intact"""
    gs = ascii_set.gs
    jobs = cell_jobs(gs, 128, 100, ascii_set.g_upm, 16, first_glyph=0, n_glyphs=95)
    got, desc = _gpu(ctx, gs, jobs, mode, (6 * 128 + 5, 2048), want=(", 1> x",))
    assert np.array_equal(got, _twin(gs, jobs, mode, got.shape)), desc
    assert (got[6 * 128:] == SENT).all()


@pytest.mark.parametrize("n,center", [(1, False), (1, True), (2, False), (2, True), (4, False), (4, True)])
def test_ascii_coverage(ctx, ascii_set, n, center):
    """DejaVuSerif-Italic's 95 glyphs in 64 x 64 cells, n x n samples (cov4_kernel / win1_kernel): == the twin"""
    gs = ascii_set.gs
    jobs = cell_jobs(gs, 64, 50, ascii_set.g_upm, 16, first_glyph=95, n_glyphs=95)
    got, desc = _gpu(ctx, gs, jobs, fr.FR_COVERAGE_U8, (6 * 64, 16 * 64), n, center)
    assert np.array_equal(got, _twin(gs, jobs, fr.FR_COVERAGE_U8, got.shape, n, center)), desc


def test_render_glyph_ex(ctx, oracle, ascii_set):
    """fr_render_glyph_ex at renderGlyph's own sizes: == the twin for every fixture glyph; STIX 'A' at 64 loses the
    reference's 29 negative windings on its baseline row and keeps every other pixel; flags = 0 is fr_render_glyph"""
    for i in range(len(ascii_set)):
        g = ascii_set.glyph(i)
        gsi = GlyphSet([g])
        upm = int(ascii_set.g_upm[i])
        size = (64, 33, 100, 17)[i % 4]
        im = rg.renderGlyphWinding(g, fr.FontInformation(upm), size, ctx=ctx, flags=FILL)
        want = FR.render_glyph(gsi.points_xy, gsi.contour_start, g.box.as_array(), upm, size, FR.WINDING_I16)
        assert np.array_equal(im.as_2d(), want), i
        gray = rg.renderGlyph(g, fr.FontInformation(upm), size, ctx=ctx, flags=FILL)
        assert np.array_equal(gray.as_2d(), FR.to_mode(want.astype(np.int32), FR.GRAY_DEBUG)), i
    i = ascii_set.find("STIX", "A")
    a_fill = rg.renderGlyphWinding(ascii_set.glyph(i), fr.FontInformation(1000), 64, ctx=ctx, flags=FILL).as_2d()
    a_ref = rg.renderGlyphWinding(ascii_set.glyph(i), fr.FontInformation(1000), 64, ctx=ctx).as_2d()
    assert (a_ref[44] < 0).sum() == 29 and not (a_fill < 0).any()
    assert np.array_equal(np.delete(a_fill, 44, 0), np.delete(a_ref, 44, 0))
    assert np.array_equal(rg.renderGlyph(ascii_set.glyph(i), fr.FontInformation(1000), 64, ctx=ctx, flags=0).as_2d(),
                          oracle.render_glyph(ascii_set.glyph(i), 1000, 64))


def test_zoomed_and_shrunk_cells(ctx, ascii_set):
    """the cells of test_gpu_parity's zoomed / shrunk case (37.5 .. 4096 pixels per font unit, and whole glyphs in a
    few pixels: rows that land exactly on vertex heights, settle loops that walk)"""
    i = ascii_set.find("STIX", "g")
    gs = GlyphSet([ascii_set.glyph(i)])
    box = gs.boxes[0].astype(np.int64)
    rows, x = [], 0
    for s, (fx, fy) in [(37.5, (0.5, 0.5)), (1000.0, (0.3, 0.6)), (4096.0, (0.52, 0.41)), (333.25, (0.1, 0.9))]:
        ux, uy = box[0] + fx * (box[2] - box[0]), box[1] + fy * (box[3] - box[1])
        rows.append((0, int(ux * s) - 30, int(uy * s) + 20, 61, 43, x, 0, np.float32(s)))
        x += 64
    for s in (0.004, 0.0009765625, 0.02, 1.0, 0.5):
        rows.append((0, int(np.floor(box[0] * s)) - 2, int(np.ceil(box[3] * s)) + 2,
                     min(int((box[2] - box[0]) * s) + 5, 600), min(int((box[3] - box[1]) * s) + 5, 48), x, 0, np.float32(s)))
        x += rows[-1][3] + 1
    jobs = rg.make_jobs(rows)
    for mode, n, center in [(fr.FR_COVERAGE_U8, 4, True), (fr.FR_COVERAGE_U8, 4, False), (fr.FR_WINDING_I16, 1, False),
                            (fr.FR_COVERAGE_U8, 2, True)]:
        got, desc = _gpu(ctx, gs, jobs, mode, (48, x), n, center)
        assert np.array_equal(got, _twin(gs, jobs, mode, got.shape, n, center)), (mode, n, center, desc)
        assert got.any()


@pytest.mark.parametrize("cell,segs", [(16, 24), (32, 32), (128, 64), (256, 96)])
def test_synthetic_cells(ctx, cell, segs):
    """synthetic glyphs in S x S cells, 16 samples per pixel and the gray map; the twin on every 7th pixel row"""
    gs = synth_glyphset(16, segs, first_index=900 + cell)
    jobs = cell_jobs(gs, cell, cell, 2048, 4)
    shape = atlas_shape(len(gs), cell, 4)
    for mode, n, center in [(fr.FR_COVERAGE_U8, 4, True), (fr.FR_GRAY_DEBUG, 1, False)]:
        got, desc = _gpu(ctx, gs, jobs, mode, shape, n, center)
        for j in jobs:
            rows = np.arange(0, cell, 7)
            assert np.array_equal(_job_view(got, j)[rows], _twin_rows(gs, j, mode, rows, n, center)), (mode, desc)


def test_overfull_rows_kmax8(ctx):
    """combs whose rays meet 80 / 12 crossings with 8 kept per sample row: the exact direct-sum fallback of
    cov4_kernel (n = 4, 2) and win1_kernel (n = 1) takes the piece's sign"""
    gl = []
    for teeth in (40, 6):
        cs, box = comb_glyph(teeth)
        gl.append(Glyph(Box(*[int(v) for v in box]), [Contour(c) for c in cs]))
    gs = GlyphSet(gl)
    jobs = cell_jobs(gs, 160, 150, 2048, 2)
    try:
        ctx.set_option("kmax", 8)
        for mode, n in [(fr.FR_COVERAGE_U8, 4), (fr.FR_COVERAGE_U8, 2), (fr.FR_WINDING_I16, 1)]:
            got, desc = _gpu(ctx, gs, jobs, mode, (161, 320), n, False)
            assert np.array_equal(got, _twin(gs, jobs, mode, got.shape, n, False)), (mode, n, desc)
    finally:
        ctx.set_option("kmax", 32)


def test_large_glyph_and_tall_cell(ctx):
    """a glyph of 800 segments (> 768: the general kernel on prepare_fill_kernel's records) and a cell of 2 400 sample
    rows (> 2048: the general kernel on in-LDS records); also with every record prepared stand-alone (fuse_prepare 0)"""
    big = synth_glyphset(1, 800, first_index=77)
    jobs = rg.make_jobs([(0, int(np.floor(big.boxes[0][0] * 0.05)) - 2, int(np.ceil(big.boxes[0][3] * 0.05)) + 2,
                          110, 110, 1, 1, np.float32(0.05))])
    mid = synth_glyphset(1, 96, first_index=4141)
    tall = rg.make_jobs([(0, int(np.floor(mid.boxes[0][0] * 0.1)) - 3, int(np.ceil(mid.boxes[0][3] * 0.3)) + 8,
                          200, 600, 3, 1, np.float32(0.3))])
    for opt in (1, 0):
        try:
            ctx.set_option("fuse_prepare", opt)
            for gs, jb, shape, n in ((big, jobs, (112, 112), 4), (big, jobs, (112, 112), 1), (mid, tall, (602, 204), 4)):
                got, desc = _gpu(ctx, gs, jb, fr.FR_COVERAGE_U8, shape, n, True, want=("render_kernel",))
                rows = np.arange(0, int(jb[0]["h"]), 5)
                assert np.array_equal(_job_view(got, jb[0])[rows], _twin_rows(gs, jb[0], fr.FR_COVERAGE_U8, rows, n, True)), desc
                assert (got[0] == SENT).all() and (got[:, 0] == SENT).all()
        finally:
            ctx.set_option("fuse_prepare", 1)
    # the glyph set's own records are the reference's again after a flagged render
    dgs = fr.DeviceGlyphSet(ctx, big)
    before = dgs.stats()
    _gpu(ctx, big, jobs, fr.FR_COVERAGE_U8, (112, 112), 4, True, dgs=dgs)
    assert dgs.stats() == before
    dgs.close()


def test_sdf_sign(ctx, ascii_set):
    """FR_SDF_U8 takes its sign from win1_kernel's sign-bit mode (and the general kernel): > 128 only inside, < 128
    only outside the twin's fill; and it moved where the two rules differ"""
    gs = ascii_set.gs
    jobs = cell_jobs(gs, 96, 80, ascii_set.g_upm, 16, first_glyph=0, n_glyphs=48)
    shape = atlas_shape(48, 96, 16)
    got, desc = _gpu(ctx, gs, jobs, fr.FR_SDF_U8, shape, 1, False, want=("win1_kernel<", ", 3, ", ", 1> x"))
    ref, _ = _gpu(ctx, gs, jobs, fr.FR_SDF_U8, shape, 1, False, flags=0)
    mask = _twin(gs, jobs, fr.FR_MASK_NONZERO, shape)
    assert not ((got > 128) & (mask == 0)).any() and not ((got < 128) & (mask == 255)).any(), desc
    assert (got != ref).any()


def test_fast_kernels_equal_general_kernel(ctx):
    """>= 2 048 synthetic 256^2 cells and the whole of DejaVuSerif-Italic: the fast kernels == every job on
    render_kernel (cov4 = 0), both flagged"""
    font = load_font("DejaVuSerif-Italic.ttf")
    gs_font, _ = font.glyphset()
    cases = [(synth_glyphset(2048, 48, first_index=5000), 256, 2048, 64, [(4, True), (2, False), (1, False)]),
             (gs_font, 96, font.information.units_per_em, 80, [(4, True), (1, False)])]
    for gs, cell, upm, size, ns in cases:
        dgs = fr.DeviceGlyphSet(ctx, gs)
        jobs = cell_jobs(gs, cell, size, upm, 32)
        shape = atlas_shape(len(gs), cell, 32)
        for n, center in ns:
            fast, desc = _gpu(ctx, gs, jobs, fr.FR_COVERAGE_U8, shape, n, center, dgs=dgs)
            try:
                ctx.set_option("cov4", 0)
                gen, gdesc = _gpu(ctx, gs, jobs, fr.FR_COVERAGE_U8, shape, n, center, dgs=dgs, want=("render_kernel",))
            finally:
                ctx.set_option("cov4", 1)
            assert "cov4_kernel" in desc or "win1_kernel" in desc, desc
            assert np.array_equal(fast, gen), (n, center, desc, gdesc)
        dgs.close()


def test_flags_zero_and_unknown_bits(ctx, ascii_set):
    """flags = 0 renders exactly what fr_plan_create's plan renders; a bit other than FR_FILL_CONSISTENT is FR_E_INVALID
    from all three _ex entry points"""
    gs = ascii_set.gs
    jobs = np.ascontiguousarray(cell_jobs(gs, 64, 50, ascii_set.g_upm, 16, first_glyph=0, n_glyphs=190))
    dgs = fr.DeviceGlyphSet(ctx, gs)
    lib = L.load_library()
    for mode, n in [(fr.FR_COVERAGE_U8, 4), (fr.FR_GRAY_DEBUG, 1)]:
        prm = L.RasterParams(mode, n, fr.FR_SAMPLE_CENTER, 0)
        a = np.full((12 * 64, 16 * 64), SENT, np.uint8)
        b = a.copy()
        L.check(lib.fr_render_batch(ctx._h, dgs._h, L.ptr(jobs), len(jobs), C.byref(prm), L.ptr(a), a.shape[1], a.shape[0]))
        L.check(lib.fr_render_batch_ex(ctx._h, dgs._h, L.ptr(jobs), len(jobs), C.byref(prm), 0, L.ptr(b), b.shape[1], b.shape[0]))
        assert np.array_equal(a, b)
        h = C.c_void_p()
        assert lib.fr_plan_create_ex(ctx._h, dgs._h, L.ptr(jobs), len(jobs), C.byref(prm), 2, C.byref(h)) == fr_E_INVALID
        assert lib.fr_render_batch_ex(ctx._h, dgs._h, L.ptr(jobs), len(jobs), C.byref(prm), 0x80000001, L.ptr(b),
                                      b.shape[1], b.shape[0]) == fr_E_INVALID
    g = ascii_set.glyph(0)
    gsi = GlyphSet([g])
    out = np.zeros(1 << 16, np.uint8)
    assert lib.fr_render_glyph_ex(ctx._h, L.ptr(gsi.points_xy), L.ptr(gsi.contour_start), gsi.n_contours, L.ptr(g.box.as_array()),
                                  1000, 20, fr.FR_GRAY_DEBUG, 4, L.ptr(out)) == fr_E_INVALID
    dgs.close()


fr_E_INVALID = -1

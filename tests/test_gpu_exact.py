"""The exact-integer kernels (fr_exact.hip: glyph_info_kernel, exact_winding_kernel with solve2 / solve1,
exact_cover_kernel, glyph_debug_color_kernel) against the Python-int reference of tests/exact_ref.py, element for
element, on every case of tests/exact_cases.py: every arm of every curve type, every outcome of both predicates,
operands up to 123 bits, glyphs of 255 / 256 / 257 / 513 curves (the staging loop's full, second and partial chunks),
query counts around one block, coverage for n = 1 .. 8 and the colour map past 255.  tests/test_exact_ref.py shows that
the cases reach all of that, and that the reference equals the C oracle on them."""
import numpy as np
import pytest

import exact_cases as EC
import font_renderer_amd as fr
from font_renderer_amd import _lib as L
from font_renderer_amd.glyph import GlyphSet

pytestmark = pytest.mark.gpu

PARTS = {"small": 3, "limit": 4, "many": 1, "coverage": 1, "colour": 1}
SENT16, SENT8 = -12345, 0xA5


def _device(ctx, j, g):
    if j.kind == "info":
        info = fr.GlyphInfo.init(g, ctx=ctx)
        return (info.curve_type, info.include_p0)
    if j.kind == "query":
        return fr.windingInGlyph(g, None, np.array(j.args[0], np.int16), ctx=ctx)
    if j.kind == "wlattice":
        return fr.winding_lattice(g, ctx=ctx)
    if j.kind == "lattice":
        return fr.exact_lattice(g, *j.args, ctx=ctx)
    if j.kind == "coverage":
        return fr.exact_coverage(g, *j.args, ctx=ctx)
    assert j.kind == "debug"
    im = fr.glyph_debug_render(g, j.args[0], ctx=ctx)
    return im.data.reshape(im.height, im.width, 3)


@pytest.mark.parametrize("name,part", [(n, p) for n in EC.TIERS for p in range(PARTS[n])])
def test_device_equals_reference(ctx, name, part):
    jobs = EC.tier(name)[0][part::PARTS[name]]
    assert 0 < len(jobs) <= 150
    glyphs = {}
    for j in jobs:
        g = glyphs.setdefault(id(j.glyph), EC.to_fr(j.glyph))
        got = _device(ctx, j, g)
        if j.kind == "info":
            assert np.array_equal(got[0], j.expect[0]) and np.array_equal(got[1], j.expect[1]), j
        else:
            assert got.dtype == j.expect.dtype and np.array_equal(got, j.expect), j


def _flat(g):
    gs = GlyphSet([g])
    return gs.points_xy, gs.contour_start, len(gs.contour_start) - 1


def test_outputs_stay_inside_their_arrays(ctx):
    """every entry point writes its result and nothing after it: sentinel-filled host arrays one row longer than needed,
    on the first job of each kind of every tier (the 64 x 64 windows and the 513-curve glyph among them)"""
    lib, h = ctx._lib, ctx._h
    for name in EC.TIERS:
        jobs, seen = EC.tier(name)[0], set()
        picks = [j for j in jobs if not (j.kind in seen or seen.add(j.kind))]
        picks += [j for j in jobs if j.kind == "lattice" and j.args[3:] == (64, 64)][:1]
        picks += [j for j in jobs if sum(len(c) // 2 for c in j.glyph) == 513 and j.kind != "info"]
        for j in picks:
            g = EC.to_fr(j.glyph)
            pts, cs, nc = _flat(g)
            box = g.box.as_array()
            if j.kind == "info":
                n = g.curve_count
                ct, ip = np.full(2 * n, SENT8, np.uint8), np.full(2 * n, SENT8, np.uint8)
                L.check(lib.fr_glyph_info_init(h, L.ptr(pts), L.ptr(cs), nc, L.ptr(ct), L.ptr(ip)))
                assert np.array_equal(ct[:n], j.expect[0]) and np.array_equal(ip[:n], j.expect[1]), j
                assert (ct[n:] == SENT8).all() and (ip[n:] == SENT8).all(), j
                continue
            rows, cols = j.expect.shape[0], int(np.prod(j.expect.shape[1:]))
            out = np.full((rows + 1, cols), SENT16 if j.expect.dtype == np.int16 else SENT8, j.expect.dtype)
            if j.kind == "query":
                q = np.ascontiguousarray(j.args[0], np.int16)
                L.check(lib.fr_winding_in_glyph(h, L.ptr(pts), L.ptr(cs), nc, L.ptr(q), len(q), L.ptr(out)))
            elif j.kind == "wlattice":
                L.check(lib.fr_winding_lattice(h, L.ptr(pts), L.ptr(cs), nc, L.ptr(box), L.ptr(out)))
            elif j.kind == "lattice":
                L.check(lib.fr_exact_lattice(h, L.ptr(pts), L.ptr(cs), nc, *j.args, L.ptr(out)))
            elif j.kind == "coverage":
                L.check(lib.fr_exact_coverage(h, L.ptr(pts), L.ptr(cs), nc, *j.args, L.ptr(out)))
            else:
                L.check(lib.fr_glyph_debug_render(h, L.ptr(pts), L.ptr(cs), nc, L.ptr(box), j.args[0], L.ptr(out)))
            assert np.array_equal(out[:rows].reshape(j.expect.shape), j.expect), j
            assert (out[rows] == out.dtype.type(SENT16 if out.dtype == np.int16 else SENT8)).all(), j


def test_empty_glyph_and_no_queries(ctx):
    lib, h = ctx._lib, ctx._h
    no_pts, no_cs = np.zeros((1, 2), np.int16), np.zeros(1, np.uint32)
    ct, ip = np.full(4, SENT8, np.uint8), np.full(4, SENT8, np.uint8)
    L.check(lib.fr_glyph_info_init(h, L.ptr(no_pts), L.ptr(no_cs), 0, L.ptr(ct), L.ptr(ip)))
    assert (ct == SENT8).all() and (ip == SENT8).all()                # no curve: nothing to write
    g = EC.to_fr(EC.small_glyphs()[0])
    pts, cs, nc = _flat(g)
    q = np.array([(0, 0), (1, 1)], np.int16)
    out = np.full(4, SENT16, np.int16)
    L.check(lib.fr_winding_in_glyph(h, L.ptr(pts), L.ptr(cs), nc, L.ptr(q), 0, L.ptr(out)))
    assert (out == SENT16).all()                                      # no query: nothing to write
    L.check(lib.fr_exact_lattice(h, L.ptr(pts), L.ptr(cs), nc, 1, 0, 0, 0, 5, L.ptr(out)))
    L.check(lib.fr_exact_lattice(h, L.ptr(pts), L.ptr(cs), nc, 8, 0, 0, 5, 0, L.ptr(out)))
    assert (out == SENT16).all()
    out8 = np.full(4, SENT8, np.uint8)
    L.check(lib.fr_exact_coverage(h, L.ptr(pts), L.ptr(cs), nc, 1, 0, 0, 0, 3, 2, L.ptr(out8)))
    assert (out8 == SENT8).all()
    # no curve but points to ask about: every winding is 0, and only those are written
    L.check(lib.fr_winding_in_glyph(h, L.ptr(no_pts), L.ptr(no_cs), 0, L.ptr(q), 2, L.ptr(out)))
    assert out.tolist() == [0, 0, SENT16, SENT16]
    out[:] = SENT16
    L.check(lib.fr_exact_lattice(h, L.ptr(no_pts), L.ptr(no_cs), 0, 8, -(1 << 20), 1 << 20, 3, 1, L.ptr(out)))
    assert out.tolist() == [0, 0, 0, SENT16]
    assert fr.GlyphInfo.init(fr.Glyph.initEmpty(), ctx=ctx).contours == []


def test_limits_are_still_refused(ctx):
    g = EC.to_fr(EC.small_glyphs()[0])
    lim = 1 << 20
    fr.exact_lattice(g, 8, -lim, lim, 2, 2, ctx=ctx)                  # the corners themselves are inside
    fr.exact_lattice(g, 8, lim - 2, -lim + 2, 2, 2, ctx=ctx)
    for args in ((9, 0, 0, 4, 4), (0, 0, 0, 4, 4), (8, -lim - 1, 0, 4, 4), (8, lim - 3, 0, 4, 4), (8, 0, lim + 1, 4, 4),
                 (8, 0, -lim + 3, 4, 4), (1, lim, 0, 1, 1)):
        with pytest.raises(fr.FrError):
            fr.exact_lattice(g, *args, ctx=ctx)
    for args in ((9, 0, 0, 4, 4, 2), (8, lim - 7, 0, 4, 4, 2), (8, 0, -lim + 7, 4, 4, 2), (1, 0, 0, 4, 4, 9), (1, 0, 0, 4, 4, 0)):
        with pytest.raises(fr.FrError):
            fr.exact_coverage(g, *args, ctx=ctx)

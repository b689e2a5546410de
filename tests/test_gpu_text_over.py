"""FR_TEXT_OVER text plans on the GPU (include/fr_raster.h): source-over alpha in every RGBA kernel family, placement form
and the mask cache.  The expected image never comes from the code under test: it is the twin assembled by
tests/text_twin.py from the twins of the plan without the flag, the exact cases of tests/text_over_cases.py, or the
definition in integers; the plan without the flag on the GPU is a second witness for R, G, B.  Outputs are
sentinel-filled (or noise under LOAD) and the whole array is compared."""
import math
import re
from contextlib import closing

import numpy as np
import pytest

import font_renderer_amd as fr
import text_block_cases as B
import text_gpu as G
import text_over_cases as OC
import text_twin as tw
from fixtures import load_font
from font_renderer_amd import _lib as L
from font_renderer_amd import render_glyph as rg
from text_gpu import BGRA, CACHE, FILL, LOAD, OVER, SRGB

pytestmark = pytest.mark.gpu
SENT = 0x5b
GRIDS = [(4, True, 0), (2, False, FILL), (1, True, 0)]                  # (n, centre phase, fill)


@pytest.fixture(scope="module")
def colour_case():
    """the shape of tests/test_gpu_text_cache.py's colour case: six overlapping italic glyphs at size 21 in two runs of
    200 x 27 with the placements in both orders, in the three placement forms; translucent colours with one A = 255 and
    one A = 0; clear colours with alpha 128 and 255; noise with random alpha for LOAD"""
    font = load_font("DejaVuSerif-Italic.ttf")
    gi, pen, _ = font.layout("fjfjWf", 21)
    gs, kept = font.glyphset(sorted({int(g) for g in gi}), skip_unsupported=False)
    local = {g: k for k, g in enumerate(kept)}
    scale = np.float32(21) / np.float32(font.information.units_per_em)
    xs = 64 * 4 + 16 + 192 * np.arange(6)
    fwd = [(local[int(g)], int(x), 20) for g, x in zip(gi, xs)]
    rows = fwd + fwd[::-1]
    plain = rg.make_places(rows)
    ex = rg.make_places_ex([(g, x, 64 * y + 24, 0.0, 0.2) for g, x, y in rows])
    c, s = math.cos(math.radians(33.0)), math.sin(math.radians(33.0))
    m = tuple(float(np.float32(v)) for v in (float(scale) * c, -float(scale) * s, float(scale) * s, float(scale) * c))
    affine = rg.make_places_affine([(g, x, 64 * y) + m for g, x, y in rows])
    runs = rg.make_runs([(0, 6, 200, 27, 1, 1, scale), (6, 6, 200, 27, 1, 29, scale)])
    shape = (57, 202)
    rng = np.random.default_rng(5)
    translucent = rng.integers(0, 256, (12, 4)).astype(np.uint8)
    translucent[0, 3], translucent[7, 3] = 255, 0
    assert ((translucent[:, 3] > 0) & (translucent[:, 3] < 255)).sum() >= 8
    opaque = translucent.copy()
    opaque[:, 3] = 255
    clears = np.array([(10, 60, 90, 128), (255, 255, 240, 255)], np.uint8)
    noise = rng.integers(0, 256, shape + (4,)).astype(np.uint8)
    return dict(gs=gs, places={"plain": plain, "ex": ex, "affine": affine}, runs=runs, shape=shape, translucent=translucent,
                opaque=opaque, clears=clears, noise=noise, sent=np.full(shape + (4,), SENT, np.uint8))


_TWINS = {}


def _twin(case, form, n, center, fill, space, load, bgra):
    """the assembled twin, computed once per combination and left unchanged"""
    key = (form, n, center, fill, space, load, bgra)
    if key not in _TWINS:
        start = case["noise"] if load else case["sent"]
        img = G.twin_rgba(form, case["gs"], case["places"][form], case["translucent"], case["runs"], None if load else case["clears"],
                          start, n, center, fill | space | load | bgra | OVER)
        img.setflags(write=False)
        _TWINS[key] = img
    return _TWINS[key]


# ---- 1. families: every space x start x placement form, three grids -------------------------------------------------------------
@pytest.mark.parametrize("form", tw.FORMS)
@pytest.mark.parametrize("load", [0, LOAD], ids=["clear", "load"])
@pytest.mark.parametrize("space", [0, SRGB], ids=["unorm", "srgb"])
def test_families_equal_the_assembled_twin(ctx, colour_case, space, load, form):
    case = colour_case
    places, cols, runs = case["places"][form], case["translucent"], case["runs"]
    clears, dst = (None, case["noise"]) if load else (case["clears"], case["sent"])
    with closing(fr.DeviceGlyphSet(ctx, case["gs"])) as dgs:
        for n, center, fill in GRIDS:
            flags = space | load | fill
            info = {}
            got = G.render_rgba(ctx, dgs, places, cols, runs, clears, dst, n, center, flags | OVER, info=info)
            assert G.kernel_name(form, flags, n, 2) in info["describe"], info
            want = _twin(case, form, n, center, fill, space, load, 0)
            assert np.array_equal(got, want), (space, load, form, n, np.argwhere(got != want)[:8].tolist())
            plain = G.render_rgba(ctx, dgs, places, cols, runs, clears, dst, n, center, flags, info=info)
            assert G.kernel_name(form, flags, n, 1) in info["describe"], info
            assert np.array_equal(got[..., :3], plain[..., :3]) and (got[..., 3] != plain[..., 3]).any()
            assert not np.array_equal(got, dst)


@pytest.mark.parametrize("space", [0, SRGB], ids=["unorm", "srgb"])
def test_bgra_once_per_space(ctx, colour_case, space):
    case = colour_case
    with closing(fr.DeviceGlyphSet(ctx, case["gs"])) as dgs:
        for form, load in (("plain", 0), ("ex", LOAD)):
            clears, dst = (None, case["noise"]) if load else (case["clears"], case["sent"])
            flags = space | load | BGRA
            info = {}
            got = G.render_rgba(ctx, dgs, case["places"][form], case["translucent"], case["runs"], clears, dst, 4, True, flags | OVER, info=info)
            assert G.kernel_name(form, flags, 4, 2) in info["describe"], info
            want = _twin(case, form, 4, True, 0, space, load, BGRA)
            assert np.array_equal(got, want), (space, form, np.argwhere(got != want)[:8].tolist())
            swapped = G.render_rgba(ctx, dgs, case["places"][form], case["translucent"], case["runs"], clears, dst, 4, True, (flags & ~BGRA) | OVER)
            assert not np.array_equal(got, swapped) and np.array_equal(got[..., 3], swapped[..., 3])


# ---- 2. the mask cache ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["plain", "ex"])
@pytest.mark.parametrize("load", [0, LOAD], ids=["clear", "load"])
@pytest.mark.parametrize("space", [0, SRGB], ids=["unorm", "srgb"])
def test_cache_equals_the_plan_without_it(ctx, colour_case, space, load, form):
    case = colour_case
    places, cols, runs = case["places"][form], case["translucent"], case["runs"]
    clears, dst = (None, case["noise"]) if load else (case["clears"], case["sent"])
    with closing(fr.DeviceGlyphSet(ctx, case["gs"])) as dgs:
        for n, center, fill in GRIDS:
            flags = space | load | fill | OVER
            info, plain = {}, {}
            got = G.render_rgba(ctx, dgs, places, cols, runs, clears, dst, n, center, flags | CACHE, info=info)
            desc = info["describe"]
            assert G.cached_kernel_name(flags, n, 2) + "12" in desc and f"fr::glyph_mask_kernel<{n}, {1 if fill else 0}> x" in desc, desc
            want = G.render_rgba(ctx, dgs, places, cols, runs, clears, dst, n, center, flags, info=plain)
            assert "cached" not in plain["describe"]
            assert np.array_equal(got, want), (space, load, form, n)
            assert np.array_equal(got, _twin(case, form, n, center, fill, space, load, 0))


def test_cache_stays_invalid_for_affine(ctx, colour_case):
    case = colour_case
    with closing(fr.DeviceGlyphSet(ctx, case["gs"])) as dgs:
        for flags in (CACHE | OVER, CACHE):
            with pytest.raises(fr.FrError) as e:
                fr.TextPlanRGBA(dgs, case["places"]["affine"], case["translucent"], case["runs"], case["clears"], 4, fr.FR_SAMPLE_CENTER, flags)
            assert e.value.code == -1


# ---- 3. opaque colours: the plan without the flag ------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", tw.FORMS)
def test_opaque_is_untouched(ctx, colour_case, form):
    case = colour_case
    places, cols, runs = case["places"][form], case["opaque"], case["runs"]
    with closing(fr.DeviceGlyphSet(ctx, case["gs"])) as dgs:
        for flags in (0, SRGB, LOAD, SRGB | LOAD):
            clears, dst = (None, case["noise"]) if flags & LOAD else (case["clears"], case["sent"])
            info, plain_info = {}, {}
            got = G.render_rgba(ctx, dgs, places, cols, runs, clears, dst, 4, True, flags | OVER, info=info)
            want = G.render_rgba(ctx, dgs, places, cols, runs, clears, dst, 4, True, flags, info=plain_info)
            desc, plain = info["describe"], plain_info["describe"]
            assert desc == plain and G.kernel_name(form, flags, 4, 0) in desc, (desc, plain)
            assert np.array_equal(got, want) and not np.array_equal(got, dst)
        if form != "affine":
            got = G.render_rgba(ctx, dgs, places, cols, runs, case["clears"], case["sent"], 2, False, CACHE | OVER | FILL, info=info)
            want = G.render_rgba(ctx, dgs, places, cols, runs, case["clears"], case["sent"], 2, False, CACHE | FILL, info=plain_info)
            desc, plain = info["describe"], plain_info["describe"]
            assert desc == plain and G.cached_kernel_name(0, 2, 0) in desc and np.array_equal(got, want)


# ---- 4. every (a, A) on the device ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("srgb", [False, True], ids=["unorm", "srgb"])
def test_every_alpha_pair(ctx, srgb):
    case = OC.every_alpha_pair_case(srgb)
    flags = LOAD | FILL | (SRGB if srgb else 0)
    with closing(fr.DeviceGlyphSet(ctx, B.glyph_set(case.glyphs))) as dgs:
        info = {}
        got = G.render_rgba(ctx, dgs, case.places, case.rgba, case.runs, None, case.start, 1, True, flags | OVER, info=info)
        plain = G.render_rgba(ctx, dgs, case.places, case.rgba, case.runs, None, case.start, 1, True, flags)
    assert G.kernel_name("plain", flags, 1, 2) + "256" in info["describe"], info
    bad = np.argwhere(got[..., 3] != case.want_alpha)
    assert not len(bad), (len(bad), bad[:8].tolist())
    assert np.array_equal(got[..., :3], plain[..., :3])
    assert np.array_equal(plain[..., 3], np.broadcast_to(np.arange(256, dtype=np.uint8)[None, :], (256, 256)))     # alpha replaced: A = k
    assert not np.array_equal(got[..., :3], case.start[..., :3])


# ---- 5. exact partial coverage -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("srgb", [False, True], ids=["unorm", "srgb"])
@pytest.mark.parametrize("ex", [False, True], ids=["place", "place_ex"])
@pytest.mark.parametrize("n", [2, 4])
def test_exact_partial_coverage(ctx, n, ex, srgb):
    case = OC.partial_cover_case(n, ex, srgb)
    flags = (SRGB if srgb else 0) | FILL
    with closing(fr.DeviceGlyphSet(ctx, B.glyph_set(case.glyphs))) as dgs:
        info = {}
        got = G.render_rgba(ctx, dgs, case.places, case.rgba, case.runs, case.clears, case.start, n, True, flags | OVER, info=info)
        assert G.kernel_name("ex" if ex else "plain", flags, n, 2) in info["describe"], info
        assert np.array_equal(got, case.want), (n, ex, srgb, np.argwhere(got != case.want)[:8].tolist())
        if not ex:
            cached = G.render_rgba(ctx, dgs, case.places, case.rgba, case.runs, case.clears, case.start, n, True, flags | OVER | CACHE, info=info)
            assert G.cached_kernel_name(flags, n, 2) in info["describe"] and np.array_equal(cached, case.want)


# ---- 6. an opaque picture stays opaque ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("srgb", [False, True], ids=["unorm", "srgb"])
def test_opaque_background_stays_opaque(ctx, srgb):
    font = load_font("DejaVuSerif-Italic.ttf")
    noise = np.random.default_rng(2).integers(0, 256, (40 * 150, 4)).astype(np.uint8)
    noise[:, 3] = 255
    ims = {}
    for over in (False, True):
        im = fr.RGBA.init(150, 40)
        im.data[:] = noise
        assert fr.draw_text_rgba(im, font, "fjord Wf", 19, 3.25, 27.5, color=(225, 105, 180, 128), srgb=srgb, over=over, ctx=ctx) is im
        ims[over] = im.data.copy()
    assert (ims[True][:, 3] == 255).all()
    assert np.array_equal(ims[True][:, :3], ims[False][:, :3]) and not np.array_equal(ims[True], noise)
    assert (ims[False][:, 3] == 128).any()                            # the alpha holes the flag removes
    layer = fr.render_text_rgba(font, "fjord Wf", 19, color=(225, 105, 180, 128), srgb=srgb, over=True, ctx=ctx)
    flat = fr.render_text_rgba(font, "fjord Wf", 19, color=(225, 105, 180, 128), srgb=srgb, ctx=ctx)
    assert np.array_equal(layer.data[:, :3], flat.data[:, :3]) and (layer.data[:, 3] >= flat.data[:, 3]).all() and flat.data[:, 3].max() <= 128
    spans = [("fj", 19, 0.2, 0.0, (10, 200, 30, 100)), ("W", 25, 0.0, 2.5, (200, 20, 30, 200))]
    a = fr.render_spans_rgba(font, spans, (10, 20, 30, 200), srgb=srgb, over=True, ctx=ctx)
    b = fr.render_spans_rgba(font, spans, (10, 20, 30, 200), srgb=srgb, ctx=ctx)
    assert np.array_equal(a.data[:, :3], b.data[:, :3]) and (a.data[:, 3] != b.data[:, 3]).any()
    a = fr.render_text_rgba_rotated(font, "fjW", 19, 30.0, 8, 50, 70, 60, color=(9, 99, 199, 77), background=(10, 20, 30, 200), srgb=srgb, over=True, ctx=ctx)
    b = fr.render_text_rgba_rotated(font, "fjW", 19, 30.0, 8, 50, 70, 60, color=(9, 99, 199, 77), background=(10, 20, 30, 200), srgb=srgb, ctx=ctx)
    assert np.array_equal(a.data[:, :3], b.data[:, :3]) and (a.data[:, 3] != b.data[:, 3]).any()
    straight = fr.RGBA(layer.width, layer.height, layer.data.copy()).unpremultiply(srgb=srgb)
    assert np.array_equal(straight.data[:, 3], layer.data[:, 3]) and (straight.data[:, :3] >= layer.data[:, :3]).all()


# ---- 7. where the flag is not taken --------------------------------------------------------------------------------------------------
def test_where_the_flag_is_not_taken(ctx, colour_case):
    case = colour_case
    with closing(fr.DeviceGlyphSet(ctx, case["gs"])) as dgs:
        for form in tw.FORMS:
            with pytest.raises(fr.FrError) as e:
                fr.TextPlan(dgs, case["places"][form], case["runs"], fr.FR_COVERAGE_U8, 4, fr.FR_SAMPLE_CENTER, OVER)
            assert e.value.code == -1, form
            for bits in (2, 16, 64, 1 << 31):                          # the unassigned bits stay unassigned beside the flag
                with pytest.raises(fr.FrError) as e:
                    fr.TextPlanRGBA(dgs, case["places"][form], case["translucent"], case["runs"], case["clears"], 4, fr.FR_SAMPLE_CENTER,
                                    OVER | bits)
                assert e.value.code == -1, (form, bits)
        jobs = rg.make_jobs([(0, 0, 20, 20, 20, 0, 0, 0.01)])
        with pytest.raises(fr.FrError) as e:
            fr.Plan(dgs, jobs, fr.FR_COVERAGE_U8, 4, fr.FR_SAMPLE_CENTER, OVER)
        assert e.value.code == -1
    lib = L.load_library()
    gsi = B.glyph_set([B.BlockGlyph("square", [B.rect(0, 0, 16, 16)])])
    box = np.array([0, 0, 16, 16], np.int16)
    out = np.zeros(1 << 12, np.uint8)
    assert lib.fr_render_glyph_ex(ctx._h, L.ptr(gsi.points_xy), L.ptr(gsi.contour_start), gsi.n_contours, L.ptr(box), 16, 20,
                                  fr.FR_GRAY_DEBUG, OVER, L.ptr(out)) == -1


# ---- 8. behaviour --------------------------------------------------------------------------------------------------------------------
def test_repeat_graph_pixels_and_stats(ctx, colour_case):
    case = colour_case
    places, cols, runs = case["places"]["plain"], case["translucent"], case["runs"]
    with closing(fr.DeviceGlyphSet(ctx, case["gs"])) as dgs:
        info, plain_info = {}, {}
        once = G.render_rgba(ctx, dgs, places, cols, runs, case["clears"], case["sent"], 4, True, OVER, info=info)
        twice = G.render_rgba(ctx, dgs, places, cols, runs, case["clears"], case["sent"], 4, True, OVER, times=2)
        assert np.array_equal(once, twice)                            # a clear colour: idempotent
        G.render_rgba(ctx, dgs, places, cols, runs, case["clears"], case["sent"], 4, True, 0, info=plain_info)
        assert all(info[k] == plain_info[k] for k in ("pixels", "stats")) and info["pixels"] == 2 * 200 * 27
        one = G.render_rgba(ctx, dgs, places, cols, runs, None, case["noise"], 4, True, OVER | LOAD)
        two = G.render_rgba(ctx, dgs, places, cols, runs, None, case["noise"], 4, True, OVER | LOAD, times=2)
        again = G.render_rgba(ctx, dgs, places, cols, runs, None, one, 4, True, OVER | LOAD)
        assert np.array_equal(two, again) and not np.array_equal(two, one)          # LOAD: the second render composites over the first
        a0, a1, a2 = (v[..., 3].astype(np.int64) for v in (case["noise"], one, two))
        assert (a1 >= a0).all() and (a2 >= a1).all() and (a2 > a1).any()           # alpha rises monotonically
        try:
            ctx.set_option("graph", 1)
            graphed = G.render_rgba(ctx, dgs, places, cols, runs, case["clears"], case["sent"], 4, True, OVER, times=2)
            graphed_cache = G.render_rgba(ctx, dgs, places, cols, runs, case["clears"], case["sent"], 4, True, OVER | CACHE, times=2)
        finally:
            ctx.set_option("graph", 0)
        assert np.array_equal(graphed, once) and np.array_equal(graphed_cache, once)
        with closing(fr.TextPlanRGBA(dgs, places, cols, runs, case["clears"], 4, fr.FR_SAMPLE_CENTER, OVER | SRGB | LOAD | BGRA)) as plan:
            assert re.fullmatch(r"fr::prepare_kernel x\d+; fr::text_srgb_load_kernel<4, 0, 2> x12", plan.describe()), plan.describe()

"""FR_TEXT_CACHE_AFFINE text plans on the GPU (include/fr_raster.h): a matrix-form plan with the flag must render, byte for
byte, what the same plan without it renders, in every family (coverage / mask, RGBA, sRGB, LOAD, OVER, BGRA), n, phase and
fill rule.  The expected image is the plan without the flag and, so that nothing rests on the GPU's own other path, the
binary32 twin of the definition (tests/text_twin.py) and the exact block-glyph images of tests/text_affine_cases.py.
Outputs are sentinel-filled (noise under LOAD) with a border, and the whole array is compared.  Every plan here carries
the new flag: the upright, _ex and raster entry points must refuse it, the two _affine ones must refuse FR_TEXT_CACHE."""
import math
import re
from contextlib import closing

import numpy as np
import pytest

import font_renderer_amd as fr
import text_affine_cases as ac
import text_block_cases as bc
import text_gpu as G
import text_twin as tw
from fixtures import load_font
from font_renderer_amd import render_glyph as rg
from text_gpu import BGRA, CACHE, FILL, LOAD, OVER, SRGB

pytestmark = pytest.mark.gpu
AFF = fr.FR_TEXT_CACHE_AFFINE
SENT = 0x5b
GRIDS = [(4, True), (4, False), (2, True), (2, False), (1, True), (1, False)]
FAMILIES = [("rgba_", 0), ("srgb_", SRGB), ("rgba_load_", LOAD), ("srgb_load_", SRGB | LOAD)]
TEXT = "minimum illumination"


def _turn(s, deg):
    c, sn = math.cos(math.radians(deg)), math.sin(math.radians(deg))
    return (s * c, -s * sn, s * sn, s * c)


def _survivors(gs, places, runs):
    """-> [(key, clipped cell, unclipped cell)] of the placements that survive clipping, in the plan's order: the key and
    the cell as include/fr_raster.h defines them, restated"""
    seg, out = gs.segments_per_glyph(), []
    for run in runs:
        for k in range(int(run["first"]), int(run["first"]) + int(run["count"])):
            g, px, py, m = tw.affine_place_params(places[k])
            if not seg[g] or not run["w"] or not run["h"]:
                continue
            c0, r0, cw, ch = tw.affine_cell(gs.boxes[g], m, px, py)
            x0, x1, y0, y1 = max(c0, 0), min(c0 + cw, int(run["w"])), max(r0, 0), min(r0 + ch, int(run["h"]))
            if x0 < x1 and y0 < y1:
                out.append(((g, px % 64, py % 64) + tuple(np.asarray(m, np.float32).view(np.uint32).tolist()), (x0, x1, y0, y1), (c0, r0, cw, ch)))
    return out


def _case(ascii_set):
    """Run 0, 200 x 100 at (3, 2): the serif f and g of the ASCII fixture at size 30 under the matrices 0, 5, 45 and 90
    degrees and a mirror, pens with every combination of a zero and a non-zero fraction, three keys used twice or more, f
    under four matrices, and placements clipped at the left, the top, and the right and bottom edges.  Run 1, 140 x 75 at
    (3, 105): the STIX m at scale 0.1, twice under one key, in a cell wider than 64 columns that is no multiple of 64 and
    of a height that is a multiple of neither 4 nor 16, the second clipped at the right edge; and three placements of f under
    the sub-pixel matrix {3 s, 0, 0, s} at size 12, two of one key."""
    gs = ascii_set.gs
    f, g, m_ = ascii_set.find("Serif", "f"), ascii_set.find("Serif", "g"), ascii_set.find("STIX", "m")
    s = float(np.float32(30) / np.float32(int(ascii_set.g_upm[f])))
    s12 = float(np.float32(12) / np.float32(int(ascii_set.g_upm[f])))
    up, five, eighth, quarter, mirror, lcd = _turn(s, 0), _turn(s, 5), _turn(s, 45), (0.0, -s, s, 0.0), (-s, 0.0, 0.0, s), (3 * s12, 0.0, 0.0, s12)
    big = (0.1, 0.0, 0.0, 0.1)                                             # (1000 units per em)
    _, _, bw, bh = tw.affine_cell(gs.boxes[m_], big, 0, 0)
    bfy = 0 if bh % 4 else 21                                              # one more row where the height is a multiple of 4
    rows = [(f, 64 * 20, 64 * 40) + up, (f, 64 * 60 + 17, 64 * 42) + up, (f, 64 * 100, 64 * 45) + up,
            (g, 64 * 130 + 9, 64 * 40 + 33) + five, (g, 64 * 165, 64 * 55 + 5) + eighth, (f, 64 * 40, 64 * 95) + quarter,
            (f, 64 * 90 + 17, 64 * 92) + mirror, (f, 64 * 120 + 3, 64 * 95 + 3) + eighth,
            (f, 64 * -3, 64 * 60) + up, (g, 64 * 196 + 9, 64 * 97 + 33) + five, (f, 64 * 150, 64 * 6) + up,
            (m_, 64 * 4, 64 * 62 + bfy) + big, (m_, 64 * 70, 64 * 66 + bfy) + big,
            (f, 64 * 10 + 11, 64 * 72) + lcd, (f, 64 * 40 + 11, 64 * 73) + lcd, (f, 64 * 60 + 12, 64 * 72) + lcd]
    places = rg.make_places_affine(rows)
    runs = rg.make_runs([(0, 11, 200, 100, 3, 2, 1.0), (11, 5, 140, 75, 3, 105, 1.0)])
    shape = (183, 207)
    sv = _survivors(gs, places, runs)
    keys = [k for k, _, _ in sv]
    assert len(sv) == len(places) == 16 and len(set(keys)) == 10, (len(sv), len(set(keys)))     # six placements read a cell another one made
    assert {(k[1] != 0, k[2] != 0) for k in keys} == {(False, False), (True, False), (False, True), (True, True)}
    assert len({k[3:] for k in keys if k[0] == f}) >= 5                    # one glyph under several matrices
    cut = set()
    for (_, (x0, x1, y0, y1), (c0, r0, cw, ch)), run in zip(sv, [runs[0]] * 11 + [runs[1]] * 5):
        cut |= {e for e, c in (("left", c0 < 0), ("top", r0 < 0), ("right", c0 + cw > run["w"]), ("bottom", r0 + ch > run["h"])) if c}
    assert cut == {"left", "top", "right", "bottom"}, cut
    _, _, bw, bh = sv[11][2]
    assert bw > 64 and bw % 64 and bh % 4 and bh % 16 and sv[12][2][2:] == (bw, bh) and sv[12][1][1] == 140, (bw, bh, sv[12])
    return gs, places, runs, shape, sv


@pytest.fixture(scope="module")
def case(ascii_set):
    gs, places, runs, shape, sv = _case(ascii_set)
    twin = {(n, center, fill): G.twin_gray("affine", gs, places, runs, shape, n, center, fill) for n, center, fill in ((4, True, True), (1, False, False))}
    return gs, places, runs, shape, sv, twin


@pytest.fixture(scope="module")
def dev(ctx, case):
    with closing(fr.DeviceGlyphSet(ctx, case[0])) as dgs:
        yield dgs


def _counts(sv):
    return len({k[0] for k, _, _ in sv}), len({k for k, _, _ in sv}), len(sv)


def _describe(sv, n, fill, composite):
    return "fr::prepare%s_kernel x%d; fr::glyph_mask_affine_kernel<%d, %d> x%d; %s x%d" % (
        ("_fill" if fill else "",) + _counts(sv)[:1] + (n, 1 if fill else 0, _counts(sv)[1], composite, _counts(sv)[2]))


# ---- 1. the same bytes as the plan without the flag; 3. fr_plan_describe --------------------------------------------------------
def test_coverage_and_mask_equal_the_plain_plan(ctx, case, dev):
    gs, places, runs, shape, sv, _ = case
    sets = [(fr.FR_COVERAGE_U8, n, center, flags) for n, center in GRIDS for flags in (0, FILL)]
    sets += [(fr.FR_MASK_NONZERO, 1, center, flags) for center in (False, True) for flags in (0, FILL)]
    assert _counts(sv) == (3, 10, 16)
    for mode, n, center, flags in sets:
        info, plain = {}, {}
        got = G.render_gray(ctx, dev, places, runs, shape, mode, n, center, flags | AFF, info=info)
        want = G.render_gray(ctx, dev, places, runs, shape, mode, n, center, flags, info=plain)
        assert np.array_equal(got, want), (mode, n, center, flags, np.argwhere(got != want)[:8].tolist())
        assert info["describe"] == _describe(sv, n, flags, "fr::text_cached_kernel<%d>" % n), info["describe"]
        assert plain["describe"].endswith("fr::text_affine_kernel<%d, %d> x16" % (n, 1 if flags else 0)) and "mask" not in plain["describe"]
        assert info["pixels"] == plain["pixels"] and info["stats"] == plain["stats"]
        assert (want[G.inside(runs, shape)] != SENT).any() and (want == 255).any() and (want[~G.inside(runs, shape)] == SENT).all()


@pytest.mark.parametrize("family,fam", FAMILIES)
def test_rgba_families_equal_the_plain_plan(ctx, case, dev, family, fam):
    gs, places, runs, shape, sv, _ = case
    clears = np.array([(10, 60, 90, 128), (255, 255, 240, 255)], np.uint8)
    dst = G.noise(shape, 5) if fam & LOAD else G.sent4(shape, SENT)
    k = 0
    for blend, over, opaque in ((0, 0, True), (1, 0, False), (2, OVER, False), (0, OVER, True)):
        cols = G.colours(len(places), 3 + blend, opaque)
        for n, center in GRIDS[k % 2::2]:                                  # each family and blend meets n = 4, 2, 1 and both phases and fills
            fill = FILL if (k + n) % 2 else 0
            k += 1
            flags = fam | over | fill | (BGRA if k % 3 == 0 else 0)
            info, plain = {}, {}
            got = G.render_rgba(ctx, dev, places, cols, runs, None if fam & LOAD else clears, dst, n, center, flags | AFF, info=info)
            want = G.render_rgba(ctx, dev, places, cols, runs, None if fam & LOAD else clears, dst, n, center, flags, info=plain)
            assert np.array_equal(got, want), (family, blend, over, n, center, fill, np.argwhere(got != want)[:8].tolist())
            assert not np.array_equal(got, dst)
            assert info["describe"] == _describe(sv, n, fill, "fr::text_cached_%skernel<%d, %d>" % (family, n, blend)), info["describe"]
            assert "fr::text_affine_%skernel<%d, %d, %d> x16" % (family, n, 1 if fill else 0, blend) in plain["describe"], plain["describe"]
            if not fam & LOAD:
                G.check_borders(got, runs, SENT)


# ---- 2. independent references ------------------------------------------------------------------------------------------------------
def test_cached_coverage_equals_the_twin(ctx, case, dev):
    gs, places, runs, shape, _, twin = case
    for (n, center, fill), want in twin.items():
        got = G.render_gray(ctx, dev, places, runs, shape, fr.FR_COVERAGE_U8, n, center, (FILL if fill else 0) | AFF)
        assert np.array_equal(got, want), (n, center, fill, np.argwhere(got != want)[:8].tolist())
        assert (want == 255).any() and (want == 0).any()


@pytest.mark.parametrize("n,center", GRIDS)
def test_block_glyph_images_are_exact(ctx, n, center):
    glyphs, places, runs, shape = ac.block_case(n, center)
    want = ac.render_runs(glyphs, places, runs, np.full(shape, SENT, np.uint8), n, center)
    with closing(fr.DeviceGlyphSet(ctx, bc.glyph_set(glyphs))) as dgs:
        info = {}
        got = G.render_gray(ctx, dgs, places, runs, shape, fr.FR_COVERAGE_U8, n, center, FILL | AFF, info=info)
    assert np.array_equal(got, want), np.argwhere(got != want)[:8]
    assert f"fr::glyph_mask_affine_kernel<{n}, 1> x" in info["describe"] and f"fr::text_cached_kernel<{n}> x" in info["describe"], info
    assert (want[2:146, 3:219] == 0).any() and (want[2:146, 3:219] == 255).any() and (want[5:12, 225:234] != 0).any()


# ---- 3. a plan whose placements are all clipped away ---------------------------------------------------------------------------------
def test_every_placement_clipped_away(ctx, case, dev):
    gs, places, runs, shape, _, _ = case
    away = places.copy()
    away["pen_x64"] += 64 * 5000
    info, plain = {}, {}
    got = G.render_gray(ctx, dev, away, runs, shape, fr.FR_COVERAGE_U8, 4, True, AFF, info=info)
    want = G.render_gray(ctx, dev, away, runs, shape, fr.FR_COVERAGE_U8, 4, True, 0, info=plain)
    assert info["describe"] == plain["describe"] == "fr::text_affine_kernel<4, 0> x0" and np.array_equal(got, want)
    assert not got[G.inside(runs, shape)].any() and (got[~G.inside(runs, shape)] == SENT).all()
    noise = G.noise(shape, 2)
    got = G.render_rgba(ctx, dev, away, G.colours(len(places), 1, True), runs, None, noise, 4, True, AFF | LOAD, info=info)
    assert np.array_equal(got, noise) and info["describe"] == ""


# ---- 4. LOAD: only the tiles some instance meets, and a second render over the first -----------------------------------------------
def test_load_tiles_and_a_second_render(ctx, case, dev):
    gs, places, runs, shape, _, _ = case
    met = tw.met_tiles("affine", gs, places, runs)
    total = sum(((int(r["w"]) + 63) // 64) * ((int(r["h"]) + 15) // 16) for r in runs)
    assert 4 <= len(met) < total
    untouched = np.ones(shape, bool)
    for r, ty, tx in met:
        run = runs[r]
        oy, ox = int(run["out_y"]), int(run["out_x"])
        untouched[oy + 16 * ty:oy + min(16 * ty + 16, int(run["h"])), ox + 64 * tx:ox + min(64 * tx + 64, int(run["w"]))] = False
    assert untouched[G.inside(runs, shape)].any()
    noise = G.noise(shape, 77)
    cols = G.colours(len(places), 21, False)
    for n, center, flags in ((4, True, LOAD), (2, False, LOAD | SRGB | FILL), (1, True, LOAD | BGRA | OVER)):
        once = {}
        for cache in (0, AFF):
            for times in (1, 2):
                once[cache, times] = G.render_rgba(ctx, dev, places, cols, runs, None, noise, n, center, flags | cache, times=times)
        assert np.array_equal(once[AFF, 1], once[0, 1]) and np.array_equal(once[AFF, 2], once[0, 2]), (n, flags)
        assert not np.array_equal(once[AFF, 2], once[AFF, 1]) and not np.array_equal(once[AFF, 1], noise)      # not idempotent: over the first
        assert np.array_equal(once[AFF, 2][untouched], noise[untouched])
    got = G.render_rgba(ctx, dev, places, cols, runs, None, noise, 2, True, LOAD | SRGB | AFF)
    assert np.array_equal(got, G.twin_rgba("affine", gs, places, cols, runs, None, noise, 2, True, LOAD | SRGB))


# ---- 5. refusals -----------------------------------------------------------------------------------------------------------------------
def _refused(ctx, buf, make):
    """`make` raises FrError -1 and the device buffer keeps its bytes"""
    with pytest.raises(fr.FrError) as e:
        make()
    ctx.sync()
    assert e.value.code == -1, e.value
    assert bool((buf == SENT).all())


def test_where_the_flags_are_not_taken(ctx, case, dev):
    import torch
    gs, places, runs, shape, _, _ = case
    buf = torch.full(shape, SENT, dtype=torch.uint8, device="cuda:0")
    cols = G.colours(len(places), 1, True)
    clears = G.colours(len(runs), 2, True)
    plain = rg.make_places([(int(p["glyph"]), int(p["pen_x64"]), int(p["pen_y64"]) >> 6) for p in places])
    ex = rg.make_places_ex([(int(p["glyph"]), int(p["pen_x64"]), int(p["pen_y64"]), 0.01, 0.0) for p in places])
    args = (fr.FR_COVERAGE_U8, 4, fr.FR_SAMPLE_CENTER)
    for pl in (plain, ex):                                                 # 512 on the upright and _ex entry points, with and without their own flag
        for flags in (AFF, AFF | CACHE, AFF | FILL):
            _refused(ctx, buf, lambda: fr.TextPlan(dev, pl, runs, *args, flags))
            _refused(ctx, buf, lambda: fr.TextPlanRGBA(dev, pl, cols, runs, clears, 4, fr.FR_SAMPLE_CENTER, flags))
    jobs = rg.make_jobs([(0, 0, 20, 20, 20, 0, 0, 0.01)])
    _refused(ctx, buf, lambda: fr.Plan(dev, jobs, *args, AFF))
    for flags in (CACHE, CACHE | AFF):                                     # 128 stays refused on the affine form, so the two together are refused everywhere
        _refused(ctx, buf, lambda: fr.TextPlan(dev, places, runs, *args, flags))
        _refused(ctx, buf, lambda: fr.TextPlanRGBA(dev, places, cols, runs, clears, 4, fr.FR_SAMPLE_CENTER, flags))
    for bits in (2, 16, 64, 1 << 31):                                      # the unassigned bits stay unassigned beside the flag
        _refused(ctx, buf, lambda: fr.TextPlan(dev, places, runs, *args, AFF | bits))
        _refused(ctx, buf, lambda: fr.TextPlanRGBA(dev, places, cols, runs, clears, 4, fr.FR_SAMPLE_CENTER, AFF | bits))
    for flags in (SRGB, BGRA, LOAD, OVER):                                 # the RGBA flags stay refused on the coverage entry point
        _refused(ctx, buf, lambda: fr.TextPlan(dev, places, runs, *args, AFF | flags))


def test_store_cap_answers_before_allocating(ctx):
    """two keys whose cells hold 40 001 x 40 001 elements (one of them a column more): FR_E_UNSUPPORTED from the host, nothing
    allocated; one of the two alone is within the limit (40 001^2 < 2^31), so the limit is the sum's"""
    import torch
    glyphs = [bc.BlockGlyph("huge", [bc.rect(0, 0, 32000, 32000)])]
    places = rg.make_places_affine([(0, 0, 64 * 50, 1.25, 0.0, 0.0, 1.25), (0, 1, 64 * 50, 1.25, 0.0, 0.0, 1.25)])
    runs = rg.make_runs([(0, 2, 100, 100, 0, 0, 1.0)])
    assert 40001 * 40001 < 2 ** 31 < 2 * 40001 * 40001
    with closing(fr.DeviceGlyphSet(ctx, bc.glyph_set(glyphs))) as dgs:
        fr.TextPlan(dgs, places, runs, fr.FR_COVERAGE_U8, 4, fr.FR_SAMPLE_CENTER, 0).close()      # fine without the flag
        torch.cuda.synchronize()
        free0, _ = torch.cuda.mem_get_info()
        with pytest.raises(fr.FrError) as e:
            fr.TextPlan(dgs, places, runs, fr.FR_COVERAGE_U8, 4, fr.FR_SAMPLE_CENTER, AFF)
        assert e.value.code == -4 and "2^31" in str(e.value), e.value
        assert torch.cuda.mem_get_info()[0] == free0


# ---- 6. the Python route ---------------------------------------------------------------------------------------------------------------
def test_python_helpers_take_cache(ctx):
    font = load_font("DejaVuSerif-Italic.ttf")
    for angle in (0.0, 33.0, 90.0):
        a = fr.render_text_rotated(font, TEXT, 15, angle, 8.3, 92.6, 180, 100, ctx=ctx)
        b = fr.render_text_rotated(font, TEXT, 15, angle, 8.3, 92.6, 180, 100, cache=True, ctx=ctx)
        assert (b.width, b.height) == (180, 100) and np.array_equal(a.data, b.data) and a.data.any(), angle
    a = fr.render_text_rgba_rotated(font, TEXT, 15, 20.0, 8.3, 92.6, 180, 100, (200, 30, 90, 140), srgb=True, over=True, ctx=ctx)
    b = fr.render_text_rgba_rotated(font, TEXT, 15, 20.0, 8.3, 92.6, 180, 100, (200, 30, 90, 140), srgb=True, over=True, cache=True, ctx=ctx)
    assert np.array_equal(a.data, b.data) and a.data.any()


@pytest.mark.parametrize("srgb", [False, True], ids=["unorm", "srgb"])
def test_lcd_text_takes_cache(ctx, srgb):
    """the plane and the image of draw_text_lcd at three thirds of a pixel: the mask fill, the composite and fr_layer_lcd
    follow each other on the stream with no sync between them"""
    font = load_font("DejaVuSans.ttf", allow_hinted=True)
    for third in range(3):
        out = []
        for cache in (False, True):
            im = fr.RGBA.init(170, 24)
            im.data[:] = (255, 255, 255, 255)
            im, plane = fr.draw_text_lcd(im, font, TEXT, 13, 3 + third / 3.0, 17.25, srgb=srgb, cache=cache, return_plane=True, ctx=ctx)
            out.append((im.data.copy(), plane.data.copy(), plane.width, plane.height))
        assert out[0][2:] == out[1][2:] == (510, 24)
        assert np.array_equal(out[0][1], out[1][1]) and out[0][1].any(), third
        assert np.array_equal(out[0][0], out[1][0]) and (out[0][0] != 255).any(), third
    im = fr.render_text_lcd(font, TEXT, 13, 3.5, 17.0, 170, 24, cache=True, ctx=ctx)
    assert np.array_equal(im.data, fr.render_text_lcd(font, TEXT, 13, 3.5, 17.0, 170, 24, ctx=ctx).data)


# ---- 7. the "graph" option ------------------------------------------------------------------------------------------------------------
def test_graph_option(ctx, case, dev):
    gs, places, runs, shape, _, _ = case
    once = G.render_gray(ctx, dev, places, runs, shape, fr.FR_COVERAGE_U8, 4, True, AFF | FILL)
    try:
        ctx.set_option("graph", 1)
        graphed = G.render_gray(ctx, dev, places, runs, shape, fr.FR_COVERAGE_U8, 4, True, AFF | FILL, times=2)
    finally:
        ctx.set_option("graph", 0)
    assert np.array_equal(graphed, once) and (once == 255).any()
    with closing(fr.TextPlan(dev, places, runs, fr.FR_COVERAGE_U8, 4, fr.FR_SAMPLE_CENTER, AFF | FILL)) as plan:
        assert re.fullmatch(r"fr::prepare_fill_kernel x3; fr::glyph_mask_affine_kernel<4, 1> x10; fr::text_cached_kernel<4> x16", plan.describe())

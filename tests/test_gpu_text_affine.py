"""Text plans of fr_glyph_place_affine placements on the GPU (fr_text_plan_create_affine / fr_text_plan_create_rgba_affine,
include/fr_raster.h): byte for byte against the fr_glyph_place_ex plans where the matrix is upright with a power-of-two
scale, against exact block-glyph images (tests/text_affine_cases.py), and against the CPU twin of the definition
(tests/text_twin.py) everywhere else.  Outputs are sentinel-filled (or, for FR_TEXT_LOAD, noise-filled) device
buffers a few pixels larger than the runs: bytes outside every run must keep what they held.  Every comparison is
np.array_equal over the whole array: the feature has no tolerance."""
import math
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
from font_renderer_amd import text as T
from text_gpu import BGRA, FILL, LOAD, SRGB

pytestmark = pytest.mark.gpu
SENT = 0x5b
GRIDS = [(4, True), (4, False), (2, True), (2, False), (1, True), (1, False)]
FAMILIES = [("rgba_", 0), ("srgb_", SRGB), ("rgba_load_", LOAD), ("srgb_load_", SRGB | LOAD)]


def _start(shape, load, seed):
    return G.noise(shape, seed) if load else G.sent4(shape, SENT)


# ---- 1. the _ex equivalence on the device (consequence 1) ----------------------------------------------------------------
@pytest.mark.parametrize("s,font_size,k,text", [(1 / 64, 32, 0.0, "ffi Tj"), (1 / 64, 32, 0.2, "Wavy /f"), (1 / 32, 64, 0.0, "fj, Ty"),
                                                (1 / 32, 64, 0.2, "gf ∫î")])
def test_upright_power_of_two_matrices_equal_the_ex_plans(ctx, s, font_size, k, text):
    font = load_font("DejaVuSerif-Italic.ttf")
    gs, places, runs, shape = tw.lines(font, [text], font_size, pad=3)
    rng = np.random.default_rng(font_size)
    ex = rg.make_places_ex([(int(p["glyph"]), int(p["pen_x64"]), 64 * int(p["pen_y"]) + int(rng.integers(1, 64)), s, k) for p in places])
    af = tw.from_ex(ex, runs)
    clears = G.colours(len(runs), 5, False)
    with closing(fr.DeviceGlyphSet(ctx, gs)) as dgs:
        for fill in (0, FILL):
            for n, center in ((1, False), (2, True), (4, True)):
                old, new = {}, {}
                a = G.render_gray(ctx, dgs, ex, runs, shape, fr.FR_COVERAGE_U8, n, center, fill, info=old)
                b = G.render_gray(ctx, dgs, af, runs, shape, fr.FR_COVERAGE_U8, n, center, fill, info=new)
                assert np.array_equal(a, b) and (a != SENT).any() and (a == SENT).any(), ("coverage", n, fill)
                assert "fr::text_place_kernel<" in old["describe"] and "fr::text_affine_kernel<" in new["describe"], (old, new)
                assert old["pixels"] == new["pixels"]
            a = G.render_gray(ctx, dgs, ex, runs, shape, fr.FR_MASK_NONZERO, 1, True, fill)
            b = G.render_gray(ctx, dgs, af, runs, shape, fr.FR_MASK_NONZERO, 1, True, fill)
            assert np.array_equal(a, b), ("mask", fill)
            n = 4 if fill else 2
            for opaque in (True, False):
                cols = G.colours(len(places), font_size + opaque, opaque)
                for flags in (0, SRGB, LOAD, SRGB | LOAD, BGRA):
                    dst = _start(shape, flags & LOAD, font_size)
                    a = G.render_rgba(ctx, dgs, ex, cols, runs, None if flags & LOAD else clears, dst, n, True, flags | fill)
                    b = G.render_rgba(ctx, dgs, af, cols, runs, None if flags & LOAD else clears, dst, n, True, flags | fill)
                    assert np.array_equal(a, b) and not np.array_equal(a, dst), ("rgba", opaque, flags, fill)


# ---- 2. exact block-glyph images under the eight maps ------------------------------------------------------------------------
@pytest.mark.parametrize("n,center", GRIDS)
def test_block_glyph_images_are_exact(ctx, n, center):
    glyphs, places, runs, shape = ac.block_case(n, center)
    want = ac.render_runs(glyphs, places, runs, np.full(shape, SENT, np.uint8), n, center)
    with closing(fr.DeviceGlyphSet(ctx, bc.glyph_set(glyphs))) as dgs:
        got = G.render_gray(ctx, dgs, places, runs, shape, fr.FR_COVERAGE_U8, n, center, FILL)
    assert np.array_equal(got, want), np.argwhere(got != want)[:8]
    assert (want[2:146, 3:219] == 0).any() and (want[2:146, 3:219] == 255).any() and (want[5:12, 225:234] != 0).any()


# ---- 3. real-font strings against the twin ------------------------------------------------------------------------------------
def _rotated(font_name, size, angle, mirror):
    font = load_font(font_name, allow_hinted=True)
    c, s = math.cos(math.radians(angle)), math.sin(math.radians(angle))
    half = 2.2 * size
    gs, places, runs = T.rotated_line(font, "Tfy jg/", size, angle, 80.3 - half * c, 48.6 + half * s, 160, 96,
                                      slant=0.2 if angle == 33 else 0.0)
    if mirror:                                                             # x -> -x in font units: a negative determinant
        places["m"][:, 0] *= -1
        places["m"][:, 2] *= -1
        places["pen_x64"] = 2 * int(places["pen_x64"].mean()) - places["pen_x64"]
    runs["out_x"], runs["out_y"] = 3, 2
    return gs, places, runs, (101, 167)


CASES = [(7, "DejaVuSans.ttf", 14, False), (33, "DejaVuSerif-Italic.ttf", 29, False), (90, "DejaVuSans.ttf", 29, False),
         (-120, "DejaVuSerif-Italic.ttf", 14, False), (33, "DejaVuSans.ttf", 29, True)]


@pytest.mark.parametrize("case", range(len(CASES)))
def test_rotated_real_font_strings_match_the_twin(ctx, case):
    angle, font_name, size, mirror = CASES[case]
    gs, places, runs, shape = _rotated(font_name, size, angle, mirror)
    m = places["m"][0].astype(np.float64)
    assert (m[0] * m[3] - m[1] * m[2] < 0) == mirror
    clears = G.colours(1, 9, False)
    with closing(fr.DeviceGlyphSet(ctx, gs)) as dgs:
        for fill in (0, FILL):
            for n, center in ((4, True), (1, False)):
                got = G.render_gray(ctx, dgs, places, runs, shape, fr.FR_COVERAGE_U8, n, center, fill)
                want = G.twin_gray("affine", gs, places, runs, shape, n, center, bool(fill))
                assert np.array_equal(got, want), ("coverage", n, fill, np.argwhere(got != want)[:8])
                inner = want[2:98, 3:163]
                assert (inner > 0).sum() > 40 * (size // 14) and (inner == 0).sum() > inner.size // 2
        for j, (_, fam) in enumerate(FAMILIES):                           # each colour family once per case; over the cases each
            n, center = ((4, True), (1, False))[(case + j) % 2]           # meets n = 4 and n = 1, both fills, opaque and not
            fill = FILL if (case + j // 2) % 2 else 0
            cols = G.colours(len(places), 10 * case + j, opaque=(case + j) % 3 == 0)
            flags = fam | fill | (BGRA if (case + j) % 4 == 3 else 0)
            dst = _start(shape, fam & LOAD, case)
            got = G.render_rgba(ctx, dgs, places, cols, runs, None if fam & LOAD else clears, dst, n, center, flags)
            want = G.twin_rgba("affine", gs, places, cols, runs, clears, dst, n, center, flags)
            assert np.array_equal(got, want), ("colour", j, n, fill, np.argwhere(got != want)[:8])
            assert not np.array_equal(got, dst)


# ---- 4. every one of the 54 instances by name -----------------------------------------------------------------------------------
def _three_glyphs():
    font = load_font("DejaVuSerif-Italic.ttf")
    gs, places, runs = T.rotated_line(font, "fgT", 24, 20.0, 12.4, 30.7, 96, 40)
    runs["out_x"], runs["out_y"] = 2, 1
    return gs, places, runs, (43, 101)


INSTANCES = [("", n, f, None) for n in (1, 2, 4) for f in (0, 1)] + [
    (fam, n, f, b) for fam, _ in FAMILIES for n in (1, 2, 4) for f in (0, 1) for b in (0, 1)]
assert len(INSTANCES) == 54


@pytest.fixture(scope="module")
def three(ctx):
    gs, places, runs, shape = _three_glyphs()
    with closing(fr.DeviceGlyphSet(ctx, gs)) as dgs:
        yield gs, dgs, places, runs, shape


@pytest.mark.parametrize("family,n,fill,blend", INSTANCES)
def test_every_affine_instance_by_name(ctx, three, family, n, fill, blend):
    gs, dgs, places, runs, shape = three
    assert len(places) == 3
    center = bool((n + fill) % 2)
    info = {}
    prep = "fr::prepare_fill_kernel x3; " if fill else "fr::prepare_kernel x3; "
    if blend is None:
        got = G.render_gray(ctx, dgs, places, runs, shape, fr.FR_COVERAGE_U8, n, center, FILL if fill else 0, info=info)
        want = G.twin_gray("affine", gs, places, runs, shape, n, center, bool(fill))
        assert info["describe"] == prep + "fr::text_affine_kernel<%d, %d> x3" % (n, fill), info
    else:
        fam = dict(FAMILIES)[family]
        flags = fam | (FILL if fill else 0)
        cols = G.colours(3, 7, opaque=not blend)
        clears = G.colours(1, 11, False)
        dst = _start(shape, fam & LOAD, n)
        got = G.render_rgba(ctx, dgs, places, cols, runs, None if fam & LOAD else clears, dst, n, center, flags, info=info)
        want = G.twin_rgba("affine", gs, places, cols, runs, clears, dst, n, center, flags)
        assert info["describe"] == prep + "fr::text_affine_%skernel<%d, %d, %d> x3" % (family, n, fill, blend), info
        assert not np.array_equal(got, dst)
    assert np.array_equal(got, want), np.argwhere(got != want)[:8]
    assert info["pixels"] == 96 * 40


# ---- 5. validation -----------------------------------------------------------------------------------------------------------------
def _code(fn):
    with pytest.raises(fr.FrError) as e:
        fn()
    return e.value.code


def test_validation_and_fully_clipped_plans(ctx, three):
    gs, dgs, places, runs, shape = three
    INVALID, UNSUPPORTED = -1, -4

    def one(m, glyph=0):
        pl = rg.make_places_affine([(glyph, 640, 640) + tuple(m)])
        r = rg.make_runs([(0, 1, 96, 40, 0, 0, 1.0)])
        return lambda: fr.TextPlan(dgs, pl, r, fr.FR_COVERAGE_U8, 4, fr.FR_SAMPLE_CENTER, 0)

    nan, inf = float("nan"), float("inf")
    for m in ((nan, 0, 0, 1), (1, 0, inf, 1), (1, -inf, 0, 1), (1, 0, 0, nan)):
        assert _code(one(m)) == INVALID, m
    for m in ((0, 0, 0, 0), (1, 2, 2, 4), (0.5, 0.5, 0.5, 0.5), (0, 0, 1, 1)):                    # D == 0
        assert _code(one(m)) == INVALID, m
    big = float(2 ** 20)
    for m in ((2 * big, 0, 0, 1), (1, 0, -2 * big, 1), (1, big + 1, 0, 1)):                        # |m| > 2^20
        assert _code(one(m)) == UNSUPPORTED, m
    for m in ((2.0 ** -21, 0, 0, 1), (1, 0, 0, -(2.0 ** -22)), (2.0 ** -12, 1.0, 0, 2.0 ** -12)):    # |q| > 2^20
        assert _code(one(m)) == UNSUPPORTED, m
    with closing(one((2.0 ** -10, 0, 0, -(2.0 ** -20)))()):                                         # |q| == 2^20 is inside; D < 0 is valid
        pass
    assert _code(one((0.01, 0, 0, 0.01), glyph=len(gs.boxes))) == INVALID                           # glyph index out of range
    ok = rg.make_places_affine([(0, 640, 640, 0.01, 0, 0, 0.01)])
    r = rg.make_runs([(0, 1, 96, 40, 0, 0, 1.0)])
    for flags in (SRGB, BGRA, LOAD):                                                                # RGBA flags on the coverage entry point
        assert _code(lambda: fr.TextPlan(dgs, ok, r, fr.FR_COVERAGE_U8, 4, fr.FR_SAMPLE_CENTER, flags)) == INVALID
    assert _code(lambda: fr.TextPlanRGBA(dgs, ok, [(1, 2, 3, 4)], r, [(0, 0, 0, 0)], 4, fr.FR_SAMPLE_CENTER, 64)) == INVALID
    assert _code(lambda: fr.TextPlan(dgs, ok, r, fr.FR_COVERAGE_U8, 3)) == UNSUPPORTED
    assert _code(lambda: fr.TextPlan(dgs, ok, rg.make_runs([(0, 1, 96, 40, 0, 0, 0.0)]))) == INVALID   # the run's scale is still validated
    # every placement clipped away: every pixel of the runs is still written, nothing else
    away = places.copy()
    away["pen_x64"] += 64 * 5000
    info = {}
    got = G.render_gray(ctx, dgs, away, runs, shape, fr.FR_COVERAGE_U8, 4, True, FILL, info=info)
    want = np.full(shape, SENT, np.uint8)
    want[1:41, 2:98] = 0
    assert np.array_equal(got, want) and info["describe"] == "fr::text_affine_kernel<4, 1> x0"
    clears = np.array([[9, 8, 7, 6]], np.uint8)
    got = G.render_rgba(ctx, dgs, away, G.colours(3, 1, False), runs, clears, _start(shape, False, 0), 2, True, SRGB)
    want = _start(shape, False, 0)
    want[1:41, 2:98] = clears[0]
    assert np.array_equal(got, want)
    dst = _start(shape, True, 3)                                                                    # LOAD: nothing is launched
    got = G.render_rgba(ctx, dgs, away, G.colours(3, 1, False), runs, None, dst, 2, True, LOAD)
    assert np.array_equal(got, dst)

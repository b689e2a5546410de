"""Text plans of fr_glyph_place_ex placements on the GPU (fr_text_plan_create_ex / fr_text_plan_create_rgba_ex,
include/fr_raster.h): byte for byte against the old entry points where the parameters are degenerate, and against the
CPU twin of the definition (tests/text_twin.py) everywhere else.  Outputs are sentinel-filled (or, for
FR_TEXT_LOAD, noise-filled) device buffers: bytes outside every run must keep what they held.  Every comparison is
np.array_equal: the feature has no tolerance."""
import ctypes as C
from contextlib import closing

import numpy as np
import pytest

import font_renderer_amd as fr
import text_gpu as G
import text_twin as tw
from fixtures import load_font
from font_renderer_amd import render_glyph as rg
from font_renderer_amd import text as T
from font_renderer_amd.glyph import GlyphSet
from font_renderer_amd.synth import synth_glyphset
from text_gpu import BGRA, FILL, LOAD, SRGB

pytestmark = pytest.mark.gpu
SENT = 0x5b
STRINGS = ["ffi fj Tf ff", "Tjfyfgf jjj", "Wavy /// fff", "ƒ∫ fî T,"]           # tests/test_gpu_text.py's STRINGS
SLANTS = [-1.0, -0.36, -0.2, 0.0, 0.2, 0.36397, 1.0, 4.0]
CONFIGS = [(4, True, 0), (4, False, FILL), (2, True, FILL), (2, False, 0), (1, True, 0), (1, False, FILL),
           (4, True, FILL), (4, False, 0), (2, True, 0), (2, False, FILL), (1, True, FILL), (1, False, 0)]


# ---- 1. old and new entry points agree -----------------------------------------------------------------------------------
@pytest.mark.parametrize("font_size,n,center", [(16, 4, True), (23, 2, False), (40, 1, True), (11, 4, False)])
def test_degenerate_placements_equal_the_old_entry_points(ctx, font_size, n, center):
    font = load_font("DejaVuSerif-Italic.ttf")
    gs, places, runs, shape = tw.lines(font, STRINGS, font_size, pad=2)
    assert any(p % 64 for p in places["pen_x64"])
    clears = G.colours(len(runs), 5, False)
    with closing(fr.DeviceGlyphSet(ctx, gs)) as dgs:
        for ex in (G.degenerate(places), G.degenerate(places, float(runs[0]["scale"]))):
            for fill in (0, FILL):
                old, new = {}, {}
                a = G.render_gray(ctx, dgs, places, runs, shape, fr.FR_COVERAGE_U8, n, center, fill, info=old)
                b = G.render_gray(ctx, dgs, ex, runs, shape, fr.FR_COVERAGE_U8, n, center, fill, info=new)
                assert np.array_equal(a, b) and (a != SENT).any(), ("coverage", fill)
                assert "fr::text_kernel<" in old["describe"] and "fr::text_place_kernel<" in new["describe"], (old, new)
                assert old["stats"] == new["stats"] and old["pixels"] == new["pixels"]
                if n == 1:
                    a = G.render_gray(ctx, dgs, places, runs, shape, fr.FR_MASK_NONZERO, 1, center, fill)
                    b = G.render_gray(ctx, dgs, ex, runs, shape, fr.FR_MASK_NONZERO, 1, center, fill)
                    assert np.array_equal(a, b), ("mask", fill)
                for opaque in (True, False):
                    cols = G.colours(len(places), font_size + opaque, opaque)
                    for flags in (0, SRGB, BGRA, SRGB | BGRA):
                        a = G.render_rgba(ctx, dgs, places, cols, runs, clears, G.sent4(shape, SENT), n, center, flags | fill)
                        b = G.render_rgba(ctx, dgs, ex, cols, runs, clears, G.sent4(shape, SENT), n, center, flags | fill)
                        assert np.array_equal(a, b), ("rgba", opaque, flags, fill)
                    dst = G.noise(shape, font_size)
                    for flags in (LOAD, LOAD | SRGB, LOAD | BGRA):
                        a = G.render_rgba(ctx, dgs, places, cols, runs, None, dst, n, center, flags | fill)
                        b = G.render_rgba(ctx, dgs, ex, cols, runs, None, dst, n, center, flags | fill)
                        assert np.array_equal(a, b) and not np.array_equal(a, dst), ("load", opaque, flags, fill)


# ---- 2. the twin: random placements over real strings ----------------------------------------------------------------------
def _random_lines(seed, size):
    """the strings' lines with every placement given its own baseline fraction, scale (a quarter to four times the run's)
    and slant; the runs grow by a margin so that the moved glyphs mostly stay inside, and some are clipped"""
    font = load_font("DejaVuSerif-Italic.ttf")
    gs, places, runs, shape = tw.lines(font, STRINGS, size, pad=2)
    rng = np.random.default_rng(seed)
    rows = []
    for k, p in enumerate(places):
        fy64 = (k + seed) % 64
        mul = np.float32(2.0 ** rng.uniform(-2.0, 2.0)) if k % 3 else np.float32(1.0)
        run_scale = np.float32(size) / np.float32(font.information.units_per_em)
        rows.append((int(p["glyph"]), int(p["pen_x64"]) + 64 * 6, 64 * (int(p["pen_y"]) + 9) + fy64,
                     0.0 if k % 5 == 0 else np.float32(run_scale * mul), SLANTS[(3 * k + seed) % len(SLANTS)]))
    runs = runs.copy()
    runs["w"] += 14
    runs["h"] += 16
    runs["out_y"] += 16 * np.arange(len(runs), dtype=np.uint32)
    return gs, rg.make_places_ex(rows), runs, (shape[0] + 16 * len(runs), shape[1] + 14)


def test_every_baseline_fraction_is_drawn():
    seen = set()
    for seed, size in [(0, 19), (32, 27)]:
        _, places, _, _ = _random_lines(seed, size)
        seen |= set((places["pen_y64"] % 64).tolist())
    assert seen == set(range(64))


@pytest.mark.parametrize("seed,size", [(0, 19), (32, 27)])
def test_random_placements_equal_the_twin(ctx, seed, size):
    gs, places, runs, shape = _random_lines(seed, size)
    assert len(set(places["slant"].tolist())) == len(SLANTS)
    with closing(fr.DeviceGlyphSet(ctx, gs)) as dgs:
        for n, center, fill in CONFIGS:
            info = {}
            got = G.render_gray(ctx, dgs, places, runs, shape, fr.FR_COVERAGE_U8, n, center, fill, info=info)
            assert f"fr::text_place_kernel<{n}, {1 if fill else 0}>" in info["describe"], info
            assert np.array_equal(got, G.twin_gray("ex", gs, places, runs, shape, n, center, bool(fill))), (n, center, fill)
        got = G.render_gray(ctx, dgs, places, runs, shape, fr.FR_MASK_NONZERO, 1, True, 0)
        assert np.array_equal(got, G.twin_gray("ex", gs, places, runs, shape, 1, True, False))


@pytest.mark.parametrize("seed,size", [(3, 21)])
def test_random_placements_rgba_equal_the_twin(ctx, seed, size):
    gs, places, runs, shape = _random_lines(seed, size)
    clears = G.colours(len(runs), 9, False)
    dst = G.noise(shape, seed)
    with closing(fr.DeviceGlyphSet(ctx, gs)) as dgs:
        for opaque in (True, False):
            cols = G.colours(len(places), seed + opaque, opaque)
            for k, (n, center, fill) in enumerate(CONFIGS):
                for flags in ((0, SRGB | BGRA, LOAD, LOAD | SRGB) if k % 2 == 0 else (SRGB, BGRA, LOAD | BGRA, LOAD | SRGB | BGRA)):
                    flags |= fill
                    info = {}
                    start = dst if flags & LOAD else G.sent4(shape, SENT)
                    got = G.render_rgba(ctx, dgs, places, cols, runs, None if flags & LOAD else clears, start, n, center, flags, info=info)
                    name = "fr::text_place_%s%skernel<%d, %d, %d>" % ("srgb_" if flags & SRGB else "rgba_", "load_" if flags & LOAD else "",
                                                                      n, 1 if fill else 0, 0 if opaque else 1)
                    assert name in info["describe"], (name, info)
                    assert np.array_equal(got, G.twin_rgba("ex", gs, places, cols, runs, clears, start, n, center, flags)), (opaque, n, center, flags)


# ---- 3. clipping -------------------------------------------------------------------------------------------------------
def _clip_case(ascii_set):
    """one glyph hanging over each edge of its run, cells whose extra column / row (fractional fx / fy) is the one clipped
    away, an instance entirely outside, a run of zero instances and a run whose instance list is empty"""
    gs = ascii_set.gs
    g = ascii_set.find("Serif", "f")
    s = np.float32(30) / np.float32(int(ascii_set.g_upm[g]))
    k = 0.36397
    c0, r0, cw, ch = tw.ex_cell(gs.boxes[g], s, k, 0, 0)                   # whole-pixel pen: cw x ch; fractional: one more
    W, H = cw + 6, ch + 6
    px, py = -64 * c0, -64 * r0                                          # the pen that puts the cell at the run's (0, 0)
    pens = [(px - 64 * (cw // 2), py + 64 * 3), (px + 64 * (W - cw // 2), py + 64 * 3),      # over the left, the right,
            (px + 64 * 3, py - 64 * (ch // 2)), (px + 64 * 3, py + 64 * (H - ch // 2)),      # the top, the bottom edge
            (px + 64 * (W - cw) + 17, py + 64 * 2),                      # the extra column is column W: clipped
            (px + 64 * 2, py + 64 * (H - ch) + 33),                      # the extra row is row H: clipped
            (px + 64 * (W - cw) + 40, py + 64 * (H - ch) + 9),           # both
            (px - 64 * (cw + 1), py), (px, py + 64 * (H + 1))]           # entirely outside: left, below
    rows = [(g, x, y, 0.0, k) for x, y in pens]
    runs = [(i, 1, W, H, 2 + (i % 3) * (W + 3), 1 + (i // 3) * (H + 2), s) for i in range(len(pens))]
    runs.append((0, 0, W, H, 2, 1 + 3 * (H + 2), s))                     # no instance at all
    runs.append((0, len(pens), 150, 2 * H, 2 + W + 3, 1 + 3 * (H + 2), s))   # all of them in one wider run
    shape = (1 + 3 * (H + 2) + 2 * H + 2, max(3 * (W + 3) + 4, 2 + W + 3 + 150 + 2))
    places, runs = rg.make_places_ex(rows), rg.make_runs(runs)
    for i, want in [(4, (W - cw, 2, cw + 1, ch)), (5, (2, H - ch, cw, ch + 1)), (6, (W - cw, H - ch, cw + 1, ch + 1))]:
        assert tw.ex_cell(gs.boxes[g], s, k, *pens[i]) == want
    return gs, places, runs, shape


def test_clipping(ctx, ascii_set):
    gs, places, runs, shape = _clip_case(ascii_set)
    outside = np.ones(shape, bool)
    for r in runs:
        outside[int(r["out_y"]):int(r["out_y"]) + int(r["h"]), int(r["out_x"]):int(r["out_x"]) + int(r["w"])] = False
    cols = G.colours(len(places), 11, False)
    clears = G.colours(len(runs), 12, False)
    with closing(fr.DeviceGlyphSet(ctx, gs)) as dgs:
        for n, center, fill in CONFIGS[:6]:
            info = {}
            got = G.render_gray(ctx, dgs, places, runs, shape, fr.FR_COVERAGE_U8, n, center, fill, info=info)
            want = G.twin_gray("ex", gs, places, runs, shape, n, center, bool(fill))
            assert np.array_equal(got, want), (n, center, fill)
            assert (got[outside] == SENT).all() and not (got[~outside] == SENT).all()
            for i in (7, 8, 9):                                          # outside / no instance: every pixel written, as 0
                r = runs[i]
                assert not got[int(r["out_y"]):int(r["out_y"]) + int(r["h"]), int(r["out_x"]):int(r["out_x"]) + int(r["w"])].any()
            # 7 visible instances in their own runs; in the wide, taller run those and the one that was below its own
            assert sum(len(tw.instance_hits("ex", gs, places, r, 1)) for r in runs) == 15
            assert info["stats"]["jobs_general"] == 15 and info["pixels"] == sum(int(r["w"]) * int(r["h"]) for r in runs), info
            got = G.render_rgba(ctx, dgs, places, cols, runs, clears, G.sent4(shape, SENT), n, center, fill | (SRGB if n == 2 else 0))
            assert np.array_equal(got, G.twin_rgba("ex", gs, places, cols, runs, clears, G.sent4(shape, SENT), n, center, fill | (SRGB if n == 2 else 0)))
            assert (got[outside] == SENT).all()
        # a plan of only the empty run renders nothing
        only = rg.make_runs([tuple(runs[9])])
        assert (G.render_gray(ctx, dgs, places, only, shape)[outside] == SENT).all()


def test_load_launches_only_the_tiles_under_a_cell(ctx, ascii_set):
    """FR_TEXT_LOAD with the sheared, per-placement-scale cells: pixels of tiles no cell meets keep their bytes, and the
    plan holds exactly the instances the twin's clipping keeps.  (fr_plan_describe reports the LOAD kernel's INSTANCE
    count, as it does for every text plan and as tests/test_gpu_text_load.py reads it; the tiles are checked through
    what they leave untouched.)"""
    gs, places, runs, shape = _clip_case(ascii_set)
    g = int(places[0]["glyph"])
    s = runs[0]["scale"]
    big = rg.make_runs([(0, 5, 700, 200, 3, 2, s)])                      # 11 x 13 tiles, five small glyphs
    rows = [(g, 64 * 40 + 13, 64 * 60 + 21, 0.0, 0.2), (g, 64 * 300, 64 * 150 + 63, np.float32(2 * s), -1.0),
            (g, 64 * 650 + 5, 64 * 40, np.float32(s / 2), 4.0), (g, 64 * 699, 64 * 199 + 32, 0.0, 0.0), (g, 64 * 900, 64 * 100, 0.0, 0.0)]
    places = rg.make_places_ex(rows)
    shape = (205, 706)
    met = tw.met_tiles("ex", gs, places, big)
    assert 4 <= len(met) < 11 * 13 // 2                                  # of the run's 11 x 13 tiles
    untouched = np.ones(shape, bool)
    for _, ty, tx in met:
        untouched[2 + 16 * ty:2 + min(16 * ty + 16, 200), 3 + 64 * tx:3 + min(64 * tx + 64, 700)] = False
    dst = G.noise(shape, 77)
    with closing(fr.DeviceGlyphSet(ctx, gs)) as dgs:
        for opaque in (True, False):
            cols = G.colours(len(places), 21, opaque)
            for n, center, flags in ((4, True, LOAD), (2, False, LOAD | SRGB | FILL), (1, True, LOAD | BGRA)):
                info = {}
                got = G.render_rgba(ctx, dgs, places, cols, big, None, dst, n, center, flags, info=info)
                assert np.array_equal(got, G.twin_rgba("ex", gs, places, cols, big, None, dst, n, center, flags)), (opaque, n, flags)
                assert np.array_equal(got[untouched], dst[untouched]) and not np.array_equal(got, dst)
                name = "fr::text_place_%sload_kernel<%d, %d, %d>" % ("srgb_" if flags & SRGB else "rgba_", n, 1 if flags & FILL else 0, 0 if opaque else 1)
                assert G.count(info["describe"], name) == 4 == info["stats"]["jobs_general"], info     # the fifth is clipped away
        # all instances clipped away: nothing is launched, the buffer stays as it is
        gone = rg.make_places_ex([(g, 64 * 900, 64 * 100, 0.0, 0.2)])
        info = {}
        got = G.render_rgba(ctx, dgs, gone, G.colours(1, 1, True), rg.make_runs([(0, 1, 700, 200, 3, 2, s)]), None, dst, 4, True, LOAD, info=info)
        assert info["describe"] == "" and np.array_equal(got, dst), info


# ---- 4. a glyph of more than 768 segments and a cell taller than 512 rows ------------------------------------------------
def test_large_glyph_and_tall_cell(ctx):
    big = synth_glyphset(1, 800, first_index=77)                       # > 768 segments
    font = load_font("DejaVuSans.ttf", allow_hinted=True)
    tall, _ = font.glyphset([font.glyph_index(ord("l")), font.glyph_index(ord("|"))], skip_unsupported=False)
    gs = GlyphSet([big.glyph(0), tall.glyph(0), tall.glyph(1)])
    s_big = np.float32(0.05)
    c0, r0, w0, h0 = tw.ex_cell(gs.boxes[0], s_big, 0.2, 0, 0)
    s_tall = np.float32(700) / np.float32(2048)                          # 'l' at 700: > 512 rows, > 2048 sample rows at n = 4
    c1, r1, w1, h1 = tw.ex_cell(gs.boxes[1], s_tall, -0.2, 0, 0)
    assert 4 * h1 > 2048 and h1 > 512
    places = rg.make_places_ex([(0, -64 * c0 + 37, -64 * r0 + 11, 0.0, 0.2), (0, -64 * c0 + 64 * 9 + 5, -64 * r0 + 64 * 4 + 50, np.float32(0.04), -0.36),
                                (1, -64 * c1 + 21, -64 * r1 + 33, 0.0, -0.2), (2, -64 * c1 + 64 * 30 + 50, -64 * r1, 0.0, 0.2)])
    runs = rg.make_runs([(0, 2, w0 + 12, h0 + 6, 0, 0, s_big), (2, 2, w1 + 60, h1 + 2, w0 + 13, 0, s_tall)])
    shape = (max(h0 + 6, h1 + 2) + 1, w0 + 13 + w1 + 61)
    with closing(fr.DeviceGlyphSet(ctx, gs)) as dgs:
        info = {}
        got = G.render_gray(ctx, dgs, places, runs, shape, fr.FR_COVERAGE_U8, 4, True, info=info)
        assert info["stats"] == {"jobs_cov4": 0, "jobs_general": 4}, info
        assert info["pixels"] == sum(int(r["w"]) * int(r["h"]) for r in runs)
        assert "fr::text_place_kernel<4, 0>" in info["describe"], info
        assert np.array_equal(got, G.twin_gray("ex", gs, places, runs, shape, 4, True))
        got = G.render_gray(ctx, dgs, places, runs, shape, fr.FR_COVERAGE_U8, 2, False, FILL, info=info)
        assert "fr::text_place_kernel<2, 1>" in info["describe"], info
        assert np.array_equal(got, G.twin_gray("ex", gs, places, runs, shape, 2, False, True))


# ---- 5. the Python surface ---------------------------------------------------------------------------------------------
def test_render_spans_equals_the_twin(ctx):
    font = load_font("DejaVuSerif-Italic.ttf")
    spans = [("E = mc", 30, 0.0, 0.0, (20, 20, 20)), ("2", 15, 0.0, 13.25, (200, 0, 0, 200)), (" is ", 30, 0.0, 0.0, (20, 20, 20)),
             ("slanted", 30, 0.36397, 0.0, (0, 0, 220)), ("x", 12, -0.2, -4.5, (0, 120, 0, 128))]
    gs, places, runs, w, h, cols = T.span_line(font, spans)
    assert len(runs) == 1 and len(set(places["scale"].tolist())) == 3
    im = fr.render_spans(font, spans, ctx=ctx)
    assert (im.width, im.height) == (w, h)
    assert np.array_equal(im.as_2d(), tw.render_run("ex", gs, places, runs[0], 4, True))
    im = fr.render_spans(font, spans, samples_per_axis=2, phase=fr.FR_SAMPLE_CORNER, flags=FILL, ctx=ctx)
    assert np.array_equal(im.as_2d(), tw.render_run("ex", gs, places, runs[0], 2, False, True))
    for srgb in (False, True):
        im = fr.render_spans_rgba(font, spans, (250, 250, 240, 255), srgb=srgb, ctx=ctx)
        want = tw.rgba_render_run("ex", gs, places, np.array(cols, np.uint8), runs[0], (250, 250, 240, 255), None, 4, True, False, srgb)
        assert np.array_equal(im.as_3d(), want), srgb


def test_render_text_slant_equals_the_twin(ctx):
    font = load_font("DejaVuSans.ttf", allow_hinted=True)
    for text, size, slant in [("Tffj fix", 27, 0.2), ("jump", 9, -0.36)]:
        gs, places, runs, w, h = T._line(font, text, size, slant)
        assert places.dtype == rg.PLACE_EX_DTYPE
        im = fr.render_text(font, text, size, slant=slant, ctx=ctx)
        assert (im.width, im.height) == (w, h)
        assert np.array_equal(im.as_2d(), tw.render_run("ex", gs, places, runs[0], 4, True))
        up = fr.render_text(font, text, size, ctx=ctx)
        assert not np.array_equal(up.as_2d(), im.as_2d()) if (up.width, up.height) == (w, h) else True
        rgba = fr.render_text_rgba(font, text, size, (10, 200, 30, 180), (255, 255, 255, 255), slant=slant, ctx=ctx)
        want = tw.rgba_render_run("ex", gs, places, np.array([(10, 200, 30, 180)] * len(text), np.uint8), runs[0], (255, 255, 255, 255), None, 4, True)
        assert np.array_equal(rgba.as_3d(), want)
    # the default is today's call: the old entry point's bytes
    gs, places, runs, shape = tw.lines(font, ["Tffj fix"], 27)
    assert np.array_equal(fr.render_text(font, "Tffj fix", 27, slant=0.0, ctx=ctx).as_2d(), tw.render_run("plain", gs, places, runs[0], 4, True))


def _draw_twin(font, text, size, img, x, y, cols, slant=0.0, n=4, center=True, srgb=False):
    gi, pen, _ = font.layout(text, size)
    gs, kept = font.glyphset(sorted({int(g) for g in gi}), skip_unsupported=False)
    local = {g: k for k, g in enumerate(kept)}
    x64, y64 = int(np.floor(64 * x + 0.5)), int(np.floor(64 * y + 0.5))
    places = rg.make_places_ex([(local[int(g)], x64 + int(p), y64, 0.0, slant) for g, p in zip(gi, pen)])
    scale = np.float32(size) / np.float32(font.information.units_per_em)
    run = rg.make_runs([(0, len(places), img.shape[1], img.shape[0], 0, 0, scale)])[0]
    return tw.rgba_render_run("ex", gs, places, np.asarray(cols, np.uint8), run, None, img, n, center, False, srgb)


def test_draw_text_rgba_fractional_baseline(ctx):
    font = load_font("DejaVuSerif-Italic.ttf")
    text = "Tffj a red word"
    hl = [(255, 0, 0, 255) if 6 <= k < 9 else (0, 0, 0, 160) for k in range(len(text))]
    base = G.noise((60, 150), 31)

    def draw(y, **kw):
        im = fr.RGBA(150, 60, base.reshape(-1, 4).copy())
        assert fr.draw_text_rgba(im, font, text, 27, 2.015625, y, colors=hl, ctx=ctx, **kw) is im
        return im.as_3d().copy()

    at = draw(10.25)
    assert np.array_equal(at, _draw_twin(font, text, 27, base, 2.015625, 10.25, hl))
    assert not np.array_equal(at, draw(10)) and not np.array_equal(at, draw(11))
    assert np.array_equal(draw(40.75, srgb=True), _draw_twin(font, text, 27, base, 2.015625, 40.75, hl, srgb=True))
    assert np.array_equal(draw(33.5, slant=0.2), _draw_twin(font, text, 27, base, 2.015625, 33.5, hl, 0.2))
    # an integral y (an int or a float) gives today's bytes: the old entry point's plan, rendered here beside it
    gi, pen, _ = font.layout(text, 27)
    gs, kept = font.glyphset(sorted({int(g) for g in gi}), skip_unsupported=False)
    local = {g: k for k, g in enumerate(kept)}
    places = rg.make_places([(local[int(g)], 129 + int(p), 10) for g, p in zip(gi, pen)])
    runs = rg.make_runs([(0, len(places), 150, 60, 0, 0, np.float32(27) / np.float32(font.information.units_per_em))])
    with closing(fr.DeviceGlyphSet(ctx, gs)) as dgs:
        old = G.render_rgba(ctx, dgs, places, np.array(hl, np.uint8), runs, None, base, 4, True, LOAD)
    assert np.array_equal(draw(10.0), old) and np.array_equal(draw(10), old)
    assert np.array_equal(old, _draw_twin(font, text, 27, base, 2.015625, 10, hl))


def test_render_text_view_equals_the_twin(ctx):
    font = load_font("DejaVuSans.ttf", allow_hinted=True)
    text = "Zoom about the cursor"
    frames = []
    for zoom, ox, oy in [(1.0, 3.3, 40.7), (1.37, -25.61, 52.125), (0.61, 40.02, 30.99)]:
        gs, places, runs = T.view_line(font, text, 24, zoom, ox, oy, 260, 70)
        im = fr.render_text_view(font, text, 24, zoom, ox, oy, 260, 70, ctx=ctx)
        assert (im.width, im.height) == (260, 70)
        assert np.array_equal(im.as_2d(), tw.render_run("ex", gs, places, runs[0], 4, True)), (zoom, ox, oy)
        assert im.as_2d().any()
        frames.append(im.as_2d().copy())
    assert not np.array_equal(frames[0], frames[1])
    # a drag by 1/64 pixel down is another image; by a whole pixel it is the same image one row lower
    a = fr.render_text_view(font, text, 24, 1.37, 10.0, 52.125, 260, 70, ctx=ctx).as_2d()
    b = fr.render_text_view(font, text, 24, 1.37, 10.0, 52.125 + 1 / 64, 260, 70, ctx=ctx).as_2d()
    c = fr.render_text_view(font, text, 24, 1.37, 10.0, 53.125, 260, 70, ctx=ctx).as_2d()
    assert not np.array_equal(a, b) and np.array_equal(c[1:], a[:-1])
    assert fr.render_text_view(font, "", 24, 1.0, 0.0, 0.0, 16, 8, ctx=ctx).as_2d().shape == (8, 16)


# ---- 6. validation -----------------------------------------------------------------------------------------------------
def test_validation(ctx):
    font = load_font("DejaVuSans.ttf", allow_hinted=True)
    gs, _ = font.glyphset([font.glyph_index(ord("A")), font.glyph_index(ord("B"))], skip_unsupported=False)
    lib, ptr = ctx._lib, fr._lib.ptr
    s = np.float32(20) / np.float32(2048)
    runs = rg.make_runs([(0, 2, 30, 20, 0, 0, s), (0, 0, 40, 40, 0, 20, s), (0, 2, 200, 100, 40, 0, s)])
    cols, clears = np.array([(225, 105, 180, 255)] * 2, np.uint8), np.zeros((3, 4), np.uint8)

    with closing(fr.DeviceGlyphSet(ctx, gs)) as dgs:
        def cov(rows, flags=0, mode=fr.FR_COVERAGE_U8, n=4, phase=fr.FR_SAMPLE_CENTER, rn=runs, null_places=False):
            places = rg.make_places_ex(rows)
            params = fr._lib.RasterParams(mode, n, phase, 0)
            h = C.c_void_p()
            rc = lib.fr_text_plan_create_ex(ctx._h, dgs._h, None if null_places else ptr(places), len(places), ptr(rn), len(rn),
                                            C.byref(params), flags, C.byref(h))
            if rc == 0:
                lib.fr_plan_destroy(h)
            else:
                assert not h.value
            return rc

        def rgba(rows, flags=0, clear=clears, n=4, mode=fr.FR_COVERAGE_U8):
            places = rg.make_places_ex(rows)
            params = fr._lib.RasterParams(mode, n, fr.FR_SAMPLE_CENTER, 0)
            h = C.c_void_p()
            rc = lib.fr_text_plan_create_rgba_ex(ctx._h, dgs._h, ptr(places), ptr(cols), len(places), ptr(runs),
                                                 None if clear is None else ptr(clear), len(runs), C.byref(params), flags, C.byref(h))
            if rc == 0:
                lib.fr_plan_destroy(h)
            return rc

        ok = [(0, 64, 64 * 16 + 5, 0.0, 0.2), (1, 700, 64 * 16, float(s) * 2, -4.0)]
        INVALID, UNSUPPORTED = -1, -4
        assert cov(ok) == 0 and rgba(ok) == 0 and cov(ok, FILL) == 0
        for both in (cov, rgba):
            # scale: 0 or finite, positive, inside [2^-20, 2^20]
            for bad, code in [(float("nan"), INVALID), (-1.0, INVALID), (float("inf"), INVALID), (-float("inf"), INVALID),
                              (2.0 ** -21, UNSUPPORTED), (2.0 ** 20 * 1.5, UNSUPPORTED)]:
                assert both([ok[0], (1, 700, 64 * 16, bad, 0.0)]) == code, bad
            assert both([ok[0], (1, 700, 64 * 16, 2.0 ** -20, 0.0)]) == 0
            # slant: finite, |k| <= 4
            for bad, code in [(float("nan"), INVALID), (float("inf"), INVALID), (4.0001, UNSUPPORTED), (-5.0, UNSUPPORTED)]:
                assert both([ok[0], (1, 700, 64 * 16, 0.0, bad)]) == code, bad
            assert both([ok[0], (1, 700, 64 * 16, 0.0, 4.0)]) == 0 and both([ok[0], (1, 700, 64 * 16, 0.0, -4.0)]) == 0
            # pens beyond +-2^22 pixels (iy and ix), a glyph index out of range
            lim = 1 << 22
            assert both([ok[0], (1, 0, 64 * (lim + 1), 0.0, 0.0)]) == UNSUPPORTED
            assert both([ok[0], (1, 0, -64 * (lim + 1), 0.0, 0.0)]) == UNSUPPORTED
            assert both([ok[0], (1, 64 * (lim + 1), 0, 0.0, 0.0)]) == UNSUPPORTED
            assert both([ok[0], (1, 0, 64 * lim + 63, 0.0, 0.0)]) == 0
            assert both([ok[0], (2, 0, 0, 0.0, 0.0)]) == INVALID
            # a sheared cell larger than 65535 columns
            assert both([ok[0], (1, 0, 0, 16.0, 4.0)]) == UNSUPPORTED
            for flags in (2, 16, 1 << 31):
                assert both(ok, flags) == INVALID, flags
        # every flag the coverage form must refuse; the RGBA form takes them
        for flags in (SRGB, BGRA, LOAD, LOAD | FILL, SRGB | BGRA):
            assert cov(ok, flags) == INVALID, flags
            assert rgba(ok, flags) == 0, flags
        assert rgba(ok, LOAD, None) == 0 and rgba(ok, 0, None) == INVALID and rgba(ok, SRGB, None) == INVALID
        # modes and sample counts as fr_text_plan_create / _rgba
        assert cov(ok, mode=fr.FR_MASK_NONZERO, n=1) == 0 and cov(ok, mode=fr.FR_MASK_NONZERO, n=2) == UNSUPPORTED
        for mode in (fr.FR_WINDING_I16, fr.FR_GRAY_DEBUG, fr.FR_SDF_U8):
            assert cov(ok, mode=mode, n=1) == UNSUPPORTED and rgba(ok, mode=mode) == UNSUPPORTED
        assert cov(ok, n=3) == UNSUPPORTED and rgba(ok, n=8) == UNSUPPORTED and rgba(ok, mode=fr.FR_MASK_NONZERO, n=1) == UNSUPPORTED
        assert cov(ok, mode=7) == INVALID and cov(ok, phase=2) == INVALID
        assert cov(ok, null_places=True) == INVALID
        over = rg.make_runs([(0, 2, 30, 20, 0, 0, s), (0, 2, 30, 20, 29, 19, s)])
        assert cov(ok, rn=over) == INVALID
        assert cov(ok, rn=rg.make_runs([(1, 2, 30, 20, 0, 0, s)])) == INVALID
        with pytest.raises(fr.FrError) as e:
            fr.TextPlan(dgs, rg.make_places_ex([ok[0], (0, 0, 0, 0.0, 4.5)]), runs[:1])
        assert e.value.code == UNSUPPORTED
    for bad in (4.5, float("nan")):
        with pytest.raises(ValueError):
            fr.render_text(font, "a", 16, slant=bad, ctx=ctx)


# ---- 7. describe strings -----------------------------------------------------------------------------------------------
def test_describe_names_the_new_kernels_and_keeps_the_old_strings(ctx):
    font = load_font("DejaVuSans.ttf", allow_hinted=True)
    gs, _ = font.glyphset([font.glyph_index(ord("A")), font.glyph_index(ord("B"))], skip_unsupported=False)
    s = np.float32(20) / np.float32(2048)
    old = rg.make_places([(0, 64, 16), (1, 700, 16)])
    new = rg.make_places_ex([(0, 64, 64 * 16 + 7, 0.0, 0.2), (1, 700, 64 * 16, 0.0, 0.0)])
    runs = rg.make_runs([(0, 2, 30, 20, 0, 0, s), (0, 0, 40, 40, 0, 20, s), (0, 2, 200, 100, 40, 0, s)])
    opaque, clears = np.array([(225, 105, 180, 255)] * 2, np.uint8), np.zeros((3, 4), np.uint8)
    translucent = np.array([(225, 105, 180, 255), (1, 2, 3, 254)], np.uint8)
    with closing(fr.DeviceGlyphSet(ctx, gs)) as dgs:
        for mode, n, flags, kernel in [(fr.FR_COVERAGE_U8, 4, 0, "text%s_kernel<4, 0>"), (fr.FR_COVERAGE_U8, 2, FILL, "text%s_kernel<2, 1>"),
                                       (fr.FR_MASK_NONZERO, 1, 0, "text%s_kernel<1, 0>")]:
            prep = "fr::prepare_fill_kernel x2; fr::" if flags & FILL else "fr::prepare_kernel x2; fr::"
            with closing(fr.TextPlan(dgs, old, runs, mode, n, fr.FR_SAMPLE_CENTER, flags)) as plan:
                assert plan.describe() == prep + kernel % "" + " x4"
            with closing(fr.TextPlan(dgs, new, runs, mode, n, fr.FR_SAMPLE_CENTER, flags)) as plan:
                assert plan.describe() == prep + kernel % "_place" + " x4"
                assert plan.pixels == 600 + 1600 + 20000 and plan.stats() == {"jobs_cov4": 0, "jobs_general": 4}
        for pc, n, flags, kernel in [(opaque, 4, 0, "text%s_rgba_kernel<4, 0, 0>"), (translucent, 2, FILL, "text%s_rgba_kernel<2, 1, 1>"),
                                     (opaque, 1, SRGB | BGRA, "text%s_srgb_kernel<1, 0, 0>"), (translucent, 4, SRGB | FILL, "text%s_srgb_kernel<4, 1, 1>"),
                                     (opaque, 4, LOAD, "text%s_rgba_load_kernel<4, 0, 0>"), (translucent, 2, LOAD | FILL, "text%s_rgba_load_kernel<2, 1, 1>"),
                                     (opaque, 1, LOAD | SRGB | BGRA | FILL, "text%s_srgb_load_kernel<1, 1, 0>"),
                                     (translucent, 4, LOAD | SRGB, "text%s_srgb_load_kernel<4, 0, 1>")]:
            prep = "fr::prepare_fill_kernel x2; fr::" if flags & FILL else "fr::prepare_kernel x2; fr::"
            with closing(fr.TextPlanRGBA(dgs, old, pc, runs, clears, n, fr.FR_SAMPLE_CENTER, flags)) as plan:
                assert plan.describe() == prep + kernel % "" + " x4", plan.describe()
            with closing(fr.TextPlanRGBA(dgs, new, pc, runs, clears, n, fr.FR_SAMPLE_CENTER, flags)) as plan:
                assert plan.describe() == prep + kernel % "_place" + " x4", plan.describe()


def test_cpp_host_mirror_makes_placement_plans(ctx, ascii_set, tmp_path):
    """fr_host::PlacedText (font-renderer_amd/host/fr_host.hpp) through host_selftest's `place` case"""
    import os
    import subprocess
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "font-renderer_amd", "host", "host_selftest")
    i = ascii_set.find("STIX", "A")
    gs1 = ascii_set.gs.subset(i, i + 1)
    gs1.points_xy.astype("<i2").tofile(tmp_path / "pts.bin")
    gs1.contour_start.astype("<u4").tofile(tmp_path / "cs.bin")
    out = subprocess.run([exe, str(tmp_path / "pts.bin"), str(tmp_path / "cs.bin"), "place"], capture_output=True, text=True,
                         env=dict(os.environ, FR_HIP_RUNTIME="system"), timeout=120)
    assert out.returncode == 0, out.stderr
    assert out.stdout.strip() == ("7200 | fr::prepare_fill_kernel x1; fr::text_place_kernel<4, 1> x2 | "
                                  "fr::prepare_kernel x1; fr::text_place_srgb_load_kernel<2, 0, 1> x2"), out.stdout

"""sRGB text plans on the GPU (fr_text_plan_create_rgba with FR_TEXT_SRGB / FR_TEXT_BGRA, include/fr_raster.h): byte for
byte against the CPU twin of the definition (tests/text_twin.py).  Outputs are device buffers filled with a 4-byte
sentinel: pixels outside every run must keep it, pixels inside are all written."""
import ctypes as C
from contextlib import closing

import numpy as np
import pytest

import font_renderer_amd as fr
import text_gpu as G
import text_twin as tw
from fixtures import load_font
from font_renderer_amd import render_glyph as rg
from font_renderer_amd.glyph import GlyphSet
from font_renderer_amd.synth import synth_glyphset
from text_gpu import BGRA, FILL, SRGB, italic  # noqa: F401

pytestmark = pytest.mark.gpu
SENT = np.array([0x5b, 0xa7, 0x13, 0xc4], np.uint8)
PINK, RED, BLUE = (225, 105, 180, 255), (230, 20, 10, 255), (20, 40, 250, 255)
CONFIGS = [(4, True, 0), (4, False, FILL), (2, True, FILL), (2, False, 0), (1, True, 0), (1, False, FILL)]


def _swapped(img, runs):
    """the pixels of the runs with bytes 0 and 2 swapped (R G B A <-> B G R A); the sentinel outside them as it is"""
    out = img.copy()
    inside = G.inside(runs, img.shape[:2])
    out[inside] = img[inside][:, [2, 1, 0, 3]]
    return out


# ---- 1. overlapping instances: opaque (BLEND = 0) and translucent (BLEND = 1), RGBA and BGRA ------------------------------
@pytest.mark.parametrize("n,center,fill", CONFIGS)
def test_overlapping_pairs_equal_the_twin(ctx, italic, n, center, fill):
    gs, places, runs, shape = italic
    clears = [(0, 0, 0, 0), (255, 255, 240, 255), (10, 60, 90, 128)]
    perm = np.arange(len(places))
    for r in runs:
        f, c = int(r["first"]), int(r["count"])
        for k in range(f, f + c - 1, 2):
            perm[k], perm[k + 1] = k + 1, k
    two = np.array([RED, BLUE] * len(places), np.uint8)[:len(places)]
    rng = np.random.default_rng(n * 10 + fill)
    translucent = rng.integers(0, 256, (len(places), 4)).astype(np.uint8)
    translucent[::5, 3] = 0
    translucent[1::5, 3] = 255
    with closing(fr.DeviceGlyphSet(ctx, gs)) as dgs:
        _overlapping_pairs(ctx, dgs, gs, places, runs, shape, n, center, fill, perm, two, translucent, clears)


def _overlapping_pairs(ctx, dgs, gs, places, runs, shape, n, center, fill, perm, two, translucent, clears):
    info = {}
    outs = {}
    for name, pl, cols, blend in [("opaque", places, two, 0), ("opaque swapped", places[perm], two[perm], 0),
                                  ("translucent", places, translucent, 1),
                                  ("translucent swapped", places[perm], translucent[perm], 1)]:
        for order in (0, BGRA):
            flags = SRGB | fill | order
            got = G.render_rgba(ctx, dgs, pl, cols, runs, clears, G.sent4(shape, SENT), n, center, flags, info=info)
            assert f"fr::text_srgb_kernel<{n}, {1 if fill else 0}, {blend}> x" in info["describe"], (name, info)
            assert np.array_equal(got, G.twin_rgba("plain", gs, pl, cols, runs, clears, G.sent4(shape, SENT), n, center, flags)), (name, n, center, flags)
            G.check_borders(got, runs, SENT)
            outs[name, order] = got
        assert np.array_equal(outs[name, BGRA], _swapped(outs[name, 0], runs))
    assert not np.array_equal(outs["opaque", 0], outs["opaque swapped", 0])
    assert not np.array_equal(outs["translucent", 0], outs["translucent swapped", 0])
    # against the UNORM plan: the alpha channel is the same; RGB differs at the edges (and for n = 1 opaque, nowhere)
    unorm = G.render_rgba(ctx, dgs, places, translucent, runs, clears, G.sent4(shape, SENT), n, center, fill)
    assert np.array_equal(unorm[..., 3], outs["translucent", 0][..., 3])
    assert not np.array_equal(unorm, outs["translucent", 0])
    unorm = G.render_rgba(ctx, dgs, places, two, runs, clears, G.sent4(shape, SENT), n, center, fill | BGRA)
    assert np.array_equal(unorm, G.twin_rgba("plain", gs, places, two, runs, clears, G.sent4(shape, SENT), n, center, fill | BGRA))
    assert np.array_equal(unorm, outs["opaque", BGRA]) == (n == 1)


# ---- 2. every sub-pixel pen --------------------------------------------------------------------------------------------
def test_every_pen_fraction(ctx):
    font = load_font("DejaVuSans.ttf", allow_hinted=True)
    gs, kept = font.glyphset([font.glyph_index(ord("M")), font.glyph_index(ord("o"))], skip_unsupported=False)
    scale = np.float32(19) / np.float32(2048)
    W, H = 40, 30
    rows = []
    for g in range(2):
        for f in range(64):
            rows.append((g, 64 * 5 + f, 22))
            rows.append((g, 64 * 6 + f + 37, 22))                 # a second instance over the first, other fraction
    places = rg.make_places(rows)
    runs = rg.make_runs([(k, 2, W, H, (k // 2 % 16) * (W + 1), (k // 32) * (H + 1), scale) for k in range(0, len(rows), 2)])
    clears = [(k % 256, 255 - k % 256, 77, 255 if k % 3 else 0) for k in range(len(runs))]
    cols = np.array([(200, 30, 60, 255 if k % 2 == 0 else 140) for k in range(len(rows))], np.uint8)
    shape = (8 * (H + 1), 16 * (W + 1))
    with closing(fr.DeviceGlyphSet(ctx, gs)) as dgs:
        for n, center, flags in [(4, True, SRGB), (1, False, SRGB | BGRA), (2, True, SRGB | FILL)]:
            got = G.render_rgba(ctx, dgs, places, cols, runs, clears, G.sent4(shape, SENT), n, center, flags)
            assert np.array_equal(got, G.twin_rgba("plain", gs, places, cols, runs, clears, G.sent4(shape, SENT), n, center, flags)), (n, center, flags)
            G.check_borders(got, runs, SENT)


# ---- 3. clipping at run borders, several runs with different clear colours --------------------------------------------
def test_borders_clipping_and_clear_colours(ctx):
    font = load_font("DejaVuSerif-Italic.ttf")
    gs, kept = font.glyphset([font.glyph_index(ord(c)) for c in "fjWQ"], skip_unsupported=False)
    scale = np.float32(30) / np.float32(2048)
    rows, runs = [], []
    W, H = 23, 19
    pens = [(-300, 20), (900, 20), (400, -3), (400, 40), (-200, -5), (1300, 45), (500, 15)]     # left, right, top, bottom
    k = 0
    for px, py in pens:
        for g in range(4):
            rows.append((g, px + 17 * g, py))
            runs.append((k, 1, W, H, 3 + (k % 8) * (W + 4), 2 + (k // 8) * (H + 3), scale))
            k += 1
    rows += [(g, 200 + 640 * g // 2, 24) for g in range(4)]
    runs.append((k, 4, 60, 30, 3, 2 + 4 * (H + 3), scale))
    runs.append((0, 0, 11, 7, 70, 2 + 4 * (H + 3), scale))       # an empty run: all its clear colour
    places, runs = rg.make_places(rows), rg.make_runs(runs)
    rng = np.random.default_rng(6)
    clears = [tuple(int(v) for v in rng.integers(1, 256, 4)) for _ in range(len(runs))]
    shape = (2 + 5 * (H + 3) + 14, 8 * (W + 4) + 9)
    variants = ((np.array([PINK] * len(rows), np.uint8), SRGB), (rng.integers(0, 256, (len(rows), 4)).astype(np.uint8), SRGB),
                (rng.integers(0, 256, (len(rows), 4)).astype(np.uint8), SRGB | BGRA | FILL))
    with closing(fr.DeviceGlyphSet(ctx, gs)) as dgs:
        for cols, flags in variants:
            got = G.render_rgba(ctx, dgs, places, cols, runs, clears, G.sent4(shape, SENT), flags=flags)
            assert np.array_equal(got, G.twin_rgba("plain", gs, places, cols, runs, clears, G.sent4(shape, SENT), flags=flags)), flags
            G.check_borders(got, runs, SENT)
            last = runs[-1]
            want = np.array(clears[-1], np.uint8)[[2, 1, 0, 3] if flags & BGRA else [0, 1, 2, 3]]
            assert (got[last["out_y"]:last["out_y"] + last["h"], last["out_x"]:last["out_x"] + last["w"]] == want).all()


# ---- 4. glyphs the fast kernels do not take -----------------------------------------------------------------------------
def test_large_glyph_and_tall_cell(ctx):
    big = synth_glyphset(1, 800, first_index=77)                       # > 768 segments
    font = load_font("DejaVuSans.ttf", allow_hinted=True)
    tall, _ = font.glyphset([font.glyph_index(ord("l")), font.glyph_index(ord("|"))], skip_unsupported=False)
    gs = GlyphSet([big.glyph(0), tall.glyph(0), tall.glyph(1)])
    s_big = np.float32(0.05)
    c0, r0, w0, h0 = tw.plain_cell(gs.boxes[0], s_big, 0, 0)
    s_tall = np.float32(700) / np.float32(2048)                          # > 2048 sample rows at n = 4
    c1, r1, w1, h1 = tw.plain_cell(gs.boxes[1], s_tall, 0, 0)
    assert 4 * h1 > 2048
    places = rg.make_places([(0, -64 * c0 + 37, -r0), (0, -64 * c0 + 64 * 9 + 5, -r0 + 4),
                             (1, -64 * c1 + 21, -r1), (2, -64 * c1 + 64 * 30 + 50, -r1)])
    runs = rg.make_runs([(0, 2, w0 + 12, h0 + 5, 0, 0, s_big), (2, 2, 120, h1 + 1, w0 + 13, 0, s_tall)])
    shape = (max(h0 + 5, h1 + 1) + 1, w0 + 13 + 121)
    cols = np.array([RED, (0, 255, 0, 100), BLUE, (255, 255, 0, 0)], np.uint8)
    clears = [(0, 0, 0, 0), (255, 255, 255, 255)]
    info = {}
    with closing(fr.DeviceGlyphSet(ctx, gs)) as dgs:
        got = G.render_rgba(ctx, dgs, places, cols, runs, clears, G.sent4(shape, SENT), 4, True, SRGB, info=info)
        assert info["stats"] == {"jobs_cov4": 0, "jobs_general": 4}, info
        assert info["pixels"] == sum(int(r["w"]) * int(r["h"]) for r in runs)
        assert "fr::text_srgb_kernel<4, 0, 1> x" in info["describe"], info
        assert np.array_equal(got, G.twin_rgba("plain", gs, places, cols, runs, clears, G.sent4(shape, SENT), 4, True, SRGB))
        got = G.render_rgba(ctx, dgs, places, cols, runs, clears, G.sent4(shape, SENT), 2, False, SRGB | FILL | BGRA, info=info)
        assert "fr::text_srgb_kernel<2, 1, 1> x" in info["describe"], info
        assert np.array_equal(got, G.twin_rgba("plain", gs, places, cols, runs, clears, G.sent4(shape, SENT), 2, False, SRGB | FILL | BGRA))


# ---- 5. thousands of runs, and the graph / overlap options ---------------------------------------------------------------
def test_many_runs_graph_and_overlap(ctx):
    font = load_font("DejaVuSerif-Italic.ttf")
    rng = np.random.default_rng(2026)
    alphabet = np.array(list("abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789ffjT.,;!? "))
    strings = ["".join(rng.choice(alphabet, int(rng.integers(3, 24)))) for _ in range(2500)]
    gs, places, runs, (H, W) = tw.lines(font, strings, 14, pad=1)
    half = len(runs) // 2
    y_off = int(runs[half]["out_y"]) - 1
    runs["out_x"][half:] += W
    runs["out_y"][half:] -= y_off
    shape = (max(H - y_off, int(runs["out_y"][half - 1] + runs["h"][half - 1] + 1)), 2 * W)
    cols = np.array([PINK if s[:k].count(" ") % 2 == 0 else (40, 200, 90, 255) for s in strings for k in range(len(s))], np.uint8)
    cols[len(cols) // 2:, 3] = 150                                    # translucent in the second half
    clears = [(0, 0, 0, 0) if r % 2 else (250, 250, 250, 255) for r in range(len(runs))]
    with closing(fr.DeviceGlyphSet(ctx, gs)) as dgs:
        _many_runs(ctx, dgs, gs, places, cols, runs, clears, shape, half, rng)


def _many_runs(ctx, dgs, gs, places, cols, runs, clears, shape, half, rng):
    base = G.render_rgba(ctx, dgs, places, cols, runs, clears, G.sent4(shape, SENT), flags=SRGB)
    G.check_borders(base, runs, SENT)
    which = sorted(rng.choice(len(runs), 40, replace=False).tolist()) + [half - 1, half, len(runs) - 1]
    want = G.twin_rgba("plain", gs, places, cols, runs, clears, G.sent4(shape, SENT), flags=SRGB, which=which)
    for r in which:
        run = runs[r]
        sl = np.s_[run["out_y"]:run["out_y"] + run["h"], run["out_x"]:run["out_x"] + run["w"]]
        assert np.array_equal(base[sl], want[sl]), r
    try:
        ctx.set_option("graph", 1)
        for _ in range(3):
            assert np.array_equal(G.render_rgba(ctx, dgs, places, cols, runs, clears, G.sent4(shape, SENT), flags=SRGB), base)
        assert np.array_equal(G.render_rgba(ctx, dgs, places, cols, runs, clears, G.sent4(shape, SENT), flags=SRGB | BGRA), _swapped(base, runs))
        ctx.set_option("graph", 0)
        for ov in (0, 2):
            ctx.set_option("overlap", ov)
            assert np.array_equal(G.render_rgba(ctx, dgs, places, cols, runs, clears, G.sent4(shape, SENT), flags=SRGB), base)
    finally:
        ctx.set_option("graph", 0)
        ctx.set_option("overlap", 1)


# ---- 6. describe strings, and the flags every other entry point rejects ------------------------------------------------------
def test_describe_and_flag_validation(ctx):
    font = load_font("DejaVuSans.ttf", allow_hinted=True)
    gs, _ = font.glyphset([font.glyph_index(ord("A")), font.glyph_index(ord("B"))], skip_unsupported=False)
    dgs = fr.DeviceGlyphSet(ctx, gs)
    s = np.float32(20) / np.float32(2048)
    places = rg.make_places([(0, 64, 16), (1, 700, 16)])
    runs = rg.make_runs([(0, 2, 30, 20, 0, 0, s)])
    cols, clears = np.array([PINK, PINK], np.uint8), np.zeros((1, 4), np.uint8)
    try:                        # (a plan or glyph set left open when an assertion fails must not outlive the context)
        _describe_and_validate(ctx, ctx._lib, dgs, gs, places, runs, cols, clears)
    finally:
        dgs.close()


def _describe_and_validate(ctx, lib, dgs, gs, places, runs, cols, clears):
    translucent = np.array([PINK, (1, 2, 3, 254)], np.uint8)
    for pc, n, phase, flags, want in [
            (cols, 4, fr.FR_SAMPLE_CENTER, SRGB, "fr::prepare_kernel x2; fr::text_srgb_kernel<4, 0, 0> x2"),
            (translucent, 2, fr.FR_SAMPLE_CORNER, SRGB | FILL, "fr::prepare_fill_kernel x2; fr::text_srgb_kernel<2, 1, 1> x2"),
            (cols, 1, fr.FR_SAMPLE_CENTER, SRGB | BGRA | FILL, "fr::prepare_fill_kernel x2; fr::text_srgb_kernel<1, 1, 0> x2"),
            (translucent, 4, fr.FR_SAMPLE_CENTER, SRGB | BGRA, "fr::prepare_kernel x2; fr::text_srgb_kernel<4, 0, 1> x2"),
            (translucent, 4, fr.FR_SAMPLE_CENTER, BGRA, "fr::prepare_kernel x2; fr::text_rgba_kernel<4, 0, 1> x2"),
            (cols, 2, fr.FR_SAMPLE_CENTER, 0, "fr::prepare_kernel x2; fr::text_rgba_kernel<2, 0, 0> x2")]:
        with closing(fr.TextPlanRGBA(dgs, places, pc, runs, clears, n, phase, flags)) as plan:
            assert plan.describe() == want, (flags, plan.describe())
            assert plan.pixels == 600 and plan.stats() == {"jobs_cov4": 0, "jobs_general": 2}
    params = fr._lib.RasterParams(fr.FR_COVERAGE_U8, 4, fr.FR_SAMPLE_CENTER, 0)
    ptr = fr._lib.ptr

    def rgba(flags):
        h = C.c_void_p()
        rc = lib.fr_text_plan_create_rgba(ctx._h, dgs._h, ptr(places), ptr(cols), len(places), ptr(runs), ptr(clears),
                                          len(runs), C.byref(params), flags, C.byref(h))
        if rc == 0:
            lib.fr_plan_destroy(h)
        return rc

    for flags in (SRGB, BGRA, SRGB | BGRA, SRGB | BGRA | FILL):
        assert rgba(flags) == 0, flags
    for flags in (2, SRGB | 2, 16, 1 << 31):                                   # bit 2 stays unassigned
        assert rgba(flags) == -1, flags
    # every other entry point that takes flags keeps rejecting the new bits
    jobs = rg.make_jobs([(0, 0, 16, 16, 16, 0, 0, s_) for s_ in [np.float32(0.01)]])
    host = np.zeros((16, 16), np.uint8)
    g = gs.glyph(0)
    for bad in (SRGB, BGRA, SRGB | FILL, BGRA | FILL):
        h = C.c_void_p()
        assert lib.fr_text_plan_create(ctx._h, dgs._h, ptr(places), len(places), ptr(runs), len(runs), C.byref(params), bad,
                                       C.byref(h)) == -1, bad
        assert lib.fr_plan_create_ex(ctx._h, dgs._h, ptr(jobs), len(jobs), C.byref(params), bad, C.byref(h)) == -1, bad
        assert lib.fr_render_batch_ex(ctx._h, dgs._h, ptr(jobs), len(jobs), C.byref(params), bad, ptr(host), 16, 16) == -1, bad
        with pytest.raises(fr.FrError) as e:
            fr.renderGlyph(g, fr.FontInformation(2048), 20, ctx=ctx, flags=bad)
        assert e.value.code == -1, bad
    assert (host == 0).all()


# ---- 7. the Python path ---------------------------------------------------------------------------------------------------
def test_render_text_rgba_srgb(ctx):
    font = load_font("DejaVuSerif-Italic.ttf")
    text = "Tffj a red word"
    gs, places, runs, shape = tw.lines(font, [text], 27)
    cols = np.array([(225, 105, 180, 255)] * len(text), np.uint8)
    im = fr.render_text_rgba(font, text, 27, srgb=True, ctx=ctx)
    assert (im.height, im.width) == shape
    assert np.array_equal(im.as_3d(), tw.rgba_render_run("plain", gs, places, cols, runs[0], (0, 0, 0, 0), None, 4, True, srgb=True))
    plain = fr.render_text_rgba(font, text, 27, ctx=ctx).as_3d()
    assert np.array_equal(im.as_3d()[..., 3], plain[..., 3]) and not np.array_equal(im.as_3d(), plain)
    hl = [(255, 0, 0, 255) if 6 <= k < 9 else (0, 0, 0, 160) for k in range(len(text))]
    im2 = fr.render_text_rgba(font, text, 27, background=(255, 255, 255, 255), colors=hl, samples_per_axis=2,
                              phase=fr.FR_SAMPLE_CORNER, srgb=True, bgra=True, ctx=ctx)
    want = tw.rgba_render_run("plain", gs, places, np.array(hl, np.uint8), runs[0], (255, 255, 255, 255), None, 2, False, srgb=True, bgr=True)
    assert np.array_equal(im2.as_3d(), want)
    im3 = fr.render_text_rgba(font, text, 27, bgra=True, ctx=ctx)
    assert np.array_equal(im3.as_3d(), plain[..., [2, 1, 0, 3]])

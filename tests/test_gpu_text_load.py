"""FR_TEXT_LOAD text plans on the GPU (fr_text_plan_create_rgba with FR_TEXT_LOAD, include/fr_raster.h): drawn over
random-noise destinations, byte for byte against the CPU twin of the definition (tests/text_twin.py), and the
consequences the definition states: untouched pixels keep their bytes, a uniform destination gives the clear-colour plan,
and a second render composites over the first."""
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
from text_gpu import BGRA, FILL, LOAD, SRGB, italic  # noqa: F401

pytestmark = pytest.mark.gpu
PINK, RED, BLUE = (225, 105, 180, 255), (230, 20, 10, 255), (20, 40, 250, 255)
CONFIGS = [(4, True, 0), (4, False, FILL), (2, True, FILL), (2, False, 0), (1, True, 0), (1, False, FILL)]


# ---- 1. overlapping instances over noise: UNORM and sRGB, opaque (BLEND = 0) and translucent (BLEND = 1), BGRA ---------
@pytest.mark.parametrize("n,center,fill", CONFIGS)
def test_overlapping_pairs_over_noise_equal_the_twin(ctx, italic, n, center, fill):
    gs, places, runs, shape = italic
    two = np.array([RED, BLUE] * len(places), np.uint8)[:len(places)]
    translucent = np.random.default_rng(n * 10 + fill).integers(0, 256, (len(places), 4)).astype(np.uint8)
    translucent[::5, 3] = 0
    translucent[1::5, 3] = 255
    dst = G.noise(shape, n + 7 * fill)
    info = {}
    with closing(fr.DeviceGlyphSet(ctx, gs)) as dgs:
        for cols, blend in ((two, 0), (translucent, 1)):
            for space in (0, SRGB):
                for order in (0, BGRA):
                    flags = LOAD | fill | space | order
                    got = G.render_rgba(ctx, dgs, places, cols, runs, None, dst, n, center, flags, info=info)
                    assert G.kernel_name("plain", flags, n, blend) in info["describe"], info
                    assert np.array_equal(got, G.twin_rgba("plain", gs, places, cols, runs, None, dst, n, center, flags)), (n, center, flags)
                    assert not np.array_equal(got, dst)


# ---- 2. every sub-pixel pen ----------------------------------------------------------------------------------------------
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
    cols = np.array([(200, 30, 60, 255 if k % 2 == 0 else 140) for k in range(len(rows))], np.uint8)
    dst = G.noise((8 * (H + 1), 16 * (W + 1)), 64)
    with closing(fr.DeviceGlyphSet(ctx, gs)) as dgs:
        for n, center, flags in [(4, True, LOAD), (1, False, LOAD | SRGB | BGRA), (2, True, LOAD | SRGB | FILL)]:
            got = G.render_rgba(ctx, dgs, places, cols, runs, None, dst, n, center, flags)
            assert np.array_equal(got, G.twin_rgba("plain", gs, places, cols, runs, None, dst, n, center, flags)), (n, center, flags)


# ---- 3. clipping at all four edges; runs whose glyphs are all clipped away, and empty runs, touch nothing -----------------
def test_clipping_and_untouched_pixels(ctx):
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
    k += 4
    runs.append((0, 0, 11, 7, 70, 2 + 4 * (H + 3), scale))       # an empty run
    rows += [(0, -64 * 80, 10), (2, 64 * 90, 10), (1, 64 * 5, -60), (3, 64 * 5, 200)]
    runs.append((k, 4, 13, 9, 90, 2 + 4 * (H + 3), scale))       # a run whose glyphs all fall outside it
    places, runs = rg.make_places(rows), rg.make_runs(runs)
    shape = (2 + 5 * (H + 3) + 14, 8 * (W + 4) + 9)
    rng = np.random.default_rng(6)
    dst = G.noise(shape, 11)
    info = {}
    variants = ((np.array([PINK] * len(rows), np.uint8), LOAD), (rng.integers(0, 256, (len(rows), 4)).astype(np.uint8), LOAD | SRGB),
                (rng.integers(0, 256, (len(rows), 4)).astype(np.uint8), LOAD | SRGB | BGRA | FILL))
    with closing(fr.DeviceGlyphSet(ctx, gs)) as dgs:
        for cols, flags in variants:
            got = G.render_rgba(ctx, dgs, places, cols, runs, None, dst, flags=flags, info=info)
            assert np.array_equal(got, G.twin_rgba("plain", gs, places, cols, runs, None, dst, flags=flags)), flags
            assert info["pixels"] == sum(int(r["w"]) * int(r["h"]) for r in runs)
            # pixels outside every clipped cell (outside the runs too) keep their bytes
            cells = np.zeros(shape, bool)
            for r in runs:
                for kk in range(int(r["first"]), int(r["first"]) + int(r["count"])):
                    pl = places[kk]
                    c0, r0, cw, ch = tw.plain_cell(gs.boxes[int(pl["glyph"])], r["scale"], int(pl["pen_x64"]), int(pl["pen_y"]))
                    x0, x1 = max(c0, 0), min(c0 + cw, int(r["w"]))
                    y0, y1 = max(r0, 0), min(r0 + ch, int(r["h"]))
                    if x0 < x1 and y0 < y1:
                        cells[r["out_y"] + y0:r["out_y"] + y1, r["out_x"] + x0:r["out_x"] + x1] = True
            assert np.array_equal(got[~cells], dst[~cells])
            assert (got[cells] != dst[cells]).any()
        # a plan of only the empty run and the all-clipped run launches nothing and leaves the buffer as it is
        only = rg.make_runs([tuple(runs[i]) for i in (len(runs) - 2, len(runs) - 1)])
        got = G.render_rgba(ctx, dgs, places, cols, only, None, dst, flags=LOAD, info=info)
        assert info["describe"] == "" and np.array_equal(got, dst), info
        # ... but checks its output as the same plan with a visible glyph does: NULL, too narrow, too short, misaligned
        need_x = max(int(r["out_x"]) + int(r["w"]) for r in only)
        need_y = max(int(r["out_y"]) + int(r["h"]) for r in only)
        with closing(fr.TextPlanRGBA(dgs, places, cols, only, None, 4, fr.FR_SAMPLE_CENTER, LOAD)) as plan:
            import torch
            buf = torch.zeros((need_y, need_x, 4), dtype=torch.uint8, device="cuda:0")
            plan.render(buf.data_ptr(), need_x, need_y)
            for ptr_, stride, rows in ((0, need_x, need_y), (buf.data_ptr(), need_x - 1, need_y),
                                       (buf.data_ptr(), need_x, need_y - 1), (buf.data_ptr() + 1, need_x, need_y)):
                with pytest.raises(fr.FrError) as e:
                    plan.render(ptr_, stride, rows)
                assert e.value.code == -1, (ptr_, stride, rows)
            ctx.sync()


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
    dst = G.noise((max(h0 + 5, h1 + 1) + 1, w0 + 13 + 121), 4)
    cols = np.array([RED, (0, 255, 0, 100), BLUE, (255, 255, 0, 0)], np.uint8)
    info = {}
    with closing(fr.DeviceGlyphSet(ctx, gs)) as dgs:
        for n, center, flags in ((4, True, LOAD | SRGB), (2, False, LOAD | FILL | BGRA)):
            got = G.render_rgba(ctx, dgs, places, cols, runs, None, dst, n, center, flags, info=info)
            assert info["stats"] == {"jobs_cov4": 0, "jobs_general": 4}, info
            assert G.kernel_name("plain", flags, n, 1) in info["describe"], info
            assert np.array_equal(got, G.twin_rgba("plain", gs, places, cols, runs, None, dst, n, center, flags)), flags


# ---- 5. consequences: a uniform destination is the clear-colour plan; two renders are the twin applied twice -------------
@pytest.mark.parametrize("space", [0, SRGB])
def test_uniform_destination_and_two_renders(ctx, italic, space):
    gs, places, runs, shape = italic
    cols = np.random.default_rng(3).integers(0, 256, (len(places), 4)).astype(np.uint8)
    clears = [(0, 0, 0, 0), (255, 255, 240, 255), (10, 60, 90, 128)]
    base = G.noise(shape, 21)
    with closing(fr.DeviceGlyphSet(ctx, gs)) as dgs:
        for n, center, fill in CONFIGS[:3]:
            for order in (0, BGRA):
                flags = space | fill | order
                plain = G.render_rgba(ctx, dgs, places, cols, runs, clears, base, n, center, flags)
                d = base.copy()                                  # Q_r in every pixel of run r, in the stored byte order
                for r, run in enumerate(runs):
                    d[run["out_y"]:run["out_y"] + run["h"], run["out_x"]:run["out_x"] + run["w"]] = \
                        np.array(clears[r], np.uint8)[[2, 1, 0, 3] if order else [0, 1, 2, 3]]
                got = G.render_rgba(ctx, dgs, places, cols, runs, None, d, n, center, flags | LOAD)
                assert np.array_equal(got, plain), (n, center, flags)
        noise = G.noise(shape, 22)
        twice = G.render_rgba(ctx, dgs, places, cols, runs, None, noise, 4, True, LOAD | space, times=2)
        once = G.twin_rgba("plain", gs, places, cols, runs, None, noise, 4, True, LOAD | space)
        assert np.array_equal(twice, G.twin_rgba("plain", gs, places, cols, runs, None, once, 4, True, LOAD | space))
        assert not np.array_equal(twice, once)


# ---- 6. many runs, and the graph option replayed into two different destinations ----------------------------------------
def test_many_runs_and_graph(ctx):
    import torch
    font = load_font("DejaVuSerif-Italic.ttf")
    rng = np.random.default_rng(2026)
    alphabet = np.array(list("abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789ffjT.,;!? "))
    strings = ["".join(rng.choice(alphabet, int(rng.integers(3, 24)))) for _ in range(1500)]
    gs, places, runs, shape = tw.lines(font, strings, 14, pad=1)
    cols = np.array([PINK if s[:k].count(" ") % 2 == 0 else (40, 200, 90, 255) for s in strings for k in range(len(s))], np.uint8)
    cols[len(cols) // 2:, 3] = 150
    which = sorted(rng.choice(len(runs), 30, replace=False).tolist()) + [len(runs) - 1]
    with closing(fr.DeviceGlyphSet(ctx, gs)) as dgs:
        a, b = G.noise(shape, 1), G.noise(shape, 2)
        want = {k: G.twin_rgba("plain", gs, places, cols, runs, None, d, 4, True, LOAD | SRGB, which=which) for k, d in (("a", a), ("b", b))}
        plan = fr.TextPlanRGBA(dgs, places, cols, runs, None, 4, fr.FR_SAMPLE_CENTER, LOAD | SRGB)
        try:
            ctx.set_option("graph", 1)
            got = {}
            for k, d in (("a", a), ("b", b), ("a", a), ("b", b)):
                buf = torch.from_numpy(d).to("cuda:0")
                torch.cuda.synchronize()
                plan.render(buf.data_ptr(), shape[1], shape[0])
                ctx.sync()
                out = buf.cpu().numpy()
                assert k not in got or np.array_equal(got[k], out), k
                got[k] = out
        finally:
            ctx.set_option("graph", 0)
            plan.close()
        for k in ("a", "b"):
            for r in which:
                run = runs[r]
                sl = np.s_[run["out_y"]:run["out_y"] + run["h"], run["out_x"]:run["out_x"] + run["w"]]
                assert np.array_equal(got[k][sl], want[k][sl]), (k, r)
        assert np.array_equal(got["a"], G.render_rgba(ctx, dgs, places, cols, runs, None, a, 4, True, LOAD | SRGB))


# ---- 7. validation and describe strings -----------------------------------------------------------------------------------
def test_validation_and_describe(ctx):
    font = load_font("DejaVuSans.ttf", allow_hinted=True)
    gs, _ = font.glyphset([font.glyph_index(ord("A")), font.glyph_index(ord("B"))], skip_unsupported=False)
    dgs = fr.DeviceGlyphSet(ctx, gs)
    try:
        _validate(ctx, ctx._lib, dgs, gs)
    finally:
        dgs.close()


def _validate(ctx, lib, dgs, gs):
    s = np.float32(20) / np.float32(2048)
    places = rg.make_places([(0, 64, 16), (1, 700, 16)])
    runs = rg.make_runs([(0, 2, 30, 20, 0, 0, s), (0, 0, 40, 40, 0, 20, s), (0, 2, 200, 100, 40, 0, s)])
    cols, clears = np.array([PINK, PINK], np.uint8), np.zeros((3, 4), np.uint8)
    translucent = np.array([PINK, (1, 2, 3, 254)], np.uint8)
    for pc, n, phase, flags, want in [
            (cols, 4, fr.FR_SAMPLE_CENTER, LOAD, "fr::prepare_kernel x2; fr::text_rgba_load_kernel<4, 0, 0> x4"),
            (translucent, 2, fr.FR_SAMPLE_CORNER, LOAD | FILL, "fr::prepare_fill_kernel x2; fr::text_rgba_load_kernel<2, 1, 1> x4"),
            (cols, 1, fr.FR_SAMPLE_CENTER, LOAD | SRGB | BGRA | FILL, "fr::prepare_fill_kernel x2; fr::text_srgb_load_kernel<1, 1, 0> x4"),
            (translucent, 4, fr.FR_SAMPLE_CENTER, LOAD | SRGB, "fr::prepare_kernel x2; fr::text_srgb_load_kernel<4, 0, 1> x4")]:
        for cl in (None, clears):                                        # the clear colours are optional, and ignored
            with closing(fr.TextPlanRGBA(dgs, places, pc, runs, cl, n, phase, flags)) as plan:
                assert plan.describe() == want, (flags, plan.describe())
                assert plan.pixels == 600 + 1600 + 20000 and plan.stats() == {"jobs_cov4": 0, "jobs_general": 4}
    params = fr._lib.RasterParams(fr.FR_COVERAGE_U8, 4, fr.FR_SAMPLE_CENTER, 0)
    ptr = fr._lib.ptr

    def rgba(flags, clear=clears):
        h = C.c_void_p()
        rc = lib.fr_text_plan_create_rgba(ctx._h, dgs._h, ptr(places), ptr(cols), len(places), ptr(runs),
                                          None if clear is None else ptr(clear), len(runs), C.byref(params), flags, C.byref(h))
        if rc == 0:
            lib.fr_plan_destroy(h)
        return rc

    for flags in (LOAD, LOAD | SRGB, LOAD | BGRA, LOAD | FILL, LOAD | SRGB | BGRA | FILL):
        assert rgba(flags) == 0 and rgba(flags, None) == 0, flags
    for flags in (0, SRGB, BGRA | FILL):
        assert rgba(flags, None) == -1, flags                          # NULL clear colours: only under FR_TEXT_LOAD
    for flags in (2, 16, 1 << 31, LOAD | 2, LOAD | 16, LOAD | (1 << 31)):
        assert rgba(flags) == -1, flags
    jobs = rg.make_jobs([(0, 0, 16, 16, 16, 0, 0, np.float32(0.01))])
    host = np.zeros((16, 16), np.uint8)
    g = gs.glyph(0)
    for bad in (LOAD, LOAD | FILL, LOAD | SRGB):
        h = C.c_void_p()
        assert lib.fr_text_plan_create(ctx._h, dgs._h, ptr(places), len(places), ptr(runs), len(runs), C.byref(params), bad,
                                       C.byref(h)) == -1, bad
        assert lib.fr_plan_create_ex(ctx._h, dgs._h, ptr(jobs), len(jobs), C.byref(params), bad, C.byref(h)) == -1, bad
        assert lib.fr_render_batch_ex(ctx._h, dgs._h, ptr(jobs), len(jobs), C.byref(params), bad, ptr(host), 16, 16) == -1, bad
        with pytest.raises(fr.FrError) as e:
            fr.renderGlyph(g, fr.FontInformation(2048), 20, ctx=ctx, flags=bad)
        assert e.value.code == -1, bad
    assert (host == 0).all()
    with pytest.raises(fr.FrError) as e:                               # without FR_TEXT_LOAD the clear colours are needed
        fr.TextPlanRGBA(dgs, places, cols, runs, None, 4, fr.FR_SAMPLE_CENTER, SRGB)
    assert e.value.code == -1


# ---- 8. the Python path: draw_text_rgba ------------------------------------------------------------------------------------
def _draw_twin(font, text, size, img, x, y, cols, n=4, center=True, srgb=False, bgr=False):
    gi, pen, _ = font.layout(text, size)
    gs, kept = font.glyphset(sorted({int(g) for g in gi}), skip_unsupported=False)
    local = {g: k for k, g in enumerate(kept)}
    x64 = int(np.floor(64 * x + 0.5))
    places = rg.make_places([(local[int(g)], x64 + int(p), y) for g, p in zip(gi, pen)])
    scale = np.float32(size) / np.float32(font.information.units_per_em)
    run = rg.make_runs([(0, len(places), img.shape[1], img.shape[0], 0, 0, scale)])[0]
    return tw.rgba_render_run("plain", gs, places, np.asarray(cols, np.uint8), run, None, img, n, center, False, srgb, bgr)


def test_draw_text_rgba(ctx):
    font = load_font("DejaVuSerif-Italic.ttf")
    text = "Tffj a red word"
    hl = [(255, 0, 0, 255) if 6 <= k < 9 else (0, 0, 0, 160) for k in range(len(text))]
    for k, (x, y) in enumerate([(-20.3, 40), (90.71875, 40), (30.5, 9), (30.0, 70), (2.015625, 33)]):   # off each edge
        base = G.noise((60, 150), 30 + k)
        im = fr.RGBA(150, 60, base.reshape(-1, 4).copy())
        assert fr.draw_text_rgba(im, font, text, 27, x, y, colors=hl, ctx=ctx) is im
        assert np.array_equal(im.as_3d(), _draw_twin(font, text, 27, base, x, y, hl)), (x, y)
        assert not np.array_equal(im.as_3d(), base)
        im = fr.RGBA(150, 60, base.reshape(-1, 4).copy())
        fr.draw_text_rgba(im, font, text, 27, x, y, samples_per_axis=2, phase=fr.FR_SAMPLE_CORNER, srgb=True, bgra=True, ctx=ctx)
        assert np.array_equal(im.as_3d(), _draw_twin(font, text, 27, base, x, y, [PINK] * len(text), 2, False, True, True))
    im = fr.RGBA(150, 60, G.noise((60, 150), 3).reshape(-1, 4))
    before = im.data.copy()
    fr.draw_text_rgba(im, font, "", 27, 5, 30, ctx=ctx)                             # nothing to draw
    fr.draw_text_rgba(im, font, "Tf", 27, 400, 30, ctx=ctx)                          # all of it outside the image
    fr.draw_text_rgba(im, font, "   ", 27, 5, 30, ctx=ctx)                           # no ink
    assert np.array_equal(im.data, before)


def test_draw_text_rgba_on_a_large_frame(ctx):
    font = load_font("DejaVuSans.ttf", allow_hinted=True)
    base = G.noise((2160, 3840), 99)
    im = fr.RGBA(3840, 2160, base.reshape(-1, 4).copy())
    text = "Caption on a 3840 x 2160 frame"
    fr.draw_text_rgba(im, font, text, 32, 1700.25, 2000, color=(255, 255, 255, 220), ctx=ctx)
    got = im.as_3d()
    changed = (got != base).any(axis=2)
    ys, xs = np.nonzero(changed)
    assert 1960 <= ys.min() and ys.max() <= 2012 and 1690 <= xs.min() and xs.max() < 1700 + 32 * len(text)
    # the twin on a window around the text: the same line shifted by whole pixels, nothing of it clipped
    y0, x0 = 1950, 1680
    want = _draw_twin(font, text, 32, base[y0:2020, x0:2400], 1700.25 - x0, 2000 - y0, [(255, 255, 255, 220)] * len(text))
    assert np.array_equal(got[y0:2020, x0:2400], want)
    outside = np.ones((2160, 3840), bool)
    outside[y0:2020, x0:2400] = False
    assert np.array_equal(got[outside], base[outside])

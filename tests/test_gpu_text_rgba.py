"""RGBA text plans on the GPU (fr_text_plan_create_rgba, include/fr_raster.h): byte for byte against the CPU twin of the
definition (tests/text_twin.py), and against the coverage of a plain text plan for white on transparent.  Outputs
are device buffers filled with a 4-byte sentinel: pixels outside every run must keep it, pixels inside are all written."""
import ctypes as C
import io
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
from text_gpu import FILL, italic  # noqa: F401

pytestmark = pytest.mark.gpu
SENT = np.array([0x5b, 0xa7, 0x13, 0xc4], np.uint8)
PINK, RED, BLUE = (225, 105, 180, 255), (230, 20, 10, 255), (20, 40, 250, 255)
CONFIGS = [(4, True, 0), (4, False, FILL), (2, True, FILL), (2, False, 0), (1, True, 0), (1, False, FILL)]


def _alternating(strings, a, b):
    """per-word colours of the runs' characters (one placement each): a for the even words of a string, b for the odd"""
    return np.array([a if s[:k].count(" ") % 2 == 0 else b for s in strings for k in range(len(s))], np.uint8)


# ---- 1. overlapping instances: opaque (BLEND = 0) and translucent (BLEND = 1) colours on the same placements ----------
@pytest.mark.parametrize("n,center,flags", CONFIGS)
def test_overlapping_pairs_equal_the_twin(ctx, italic, n, center, flags):
    gs, places, runs, shape = italic
    clears = [(0, 0, 0, 0), (255, 255, 240, 255), (10, 60, 90, 128)]
    # neighbours in two colours; then the same (placement, colour) pairs in the other order
    perm = np.arange(len(places))
    for r in runs:
        f, c = int(r["first"]), int(r["count"])
        for k in range(f, f + c - 1, 2):
            perm[k], perm[k + 1] = k + 1, k
    two = np.array([RED, BLUE] * len(places), np.uint8)[:len(places)]
    rng = np.random.default_rng(n * 10 + flags)
    translucent = rng.integers(0, 256, (len(places), 4)).astype(np.uint8)
    translucent[::5, 3] = 0
    translucent[1::5, 3] = 255
    dgs = fr.DeviceGlyphSet(ctx, gs)
    info = {}
    outs = {}
    for name, pl, cols, blend in [("opaque", places, two, 0), ("opaque swapped", places[perm], two[perm], 0),
                                  ("translucent", places, translucent, 1),
                                  ("translucent swapped", places[perm], translucent[perm], 1)]:
        got = G.render_rgba(ctx, dgs, pl, cols, runs, clears, G.sent4(shape, SENT), n, center, flags, info=info)
        assert f"fr::text_rgba_kernel<{n}, {1 if flags else 0}, {blend}> x" in info["describe"], (name, info)
        assert np.array_equal(got, G.twin_rgba("plain", gs, pl, cols, runs, clears, G.sent4(shape, SENT), n, center, flags)), (name, n, center, flags)
        G.check_borders(got, runs, SENT)
        outs[name] = got
    assert not np.array_equal(outs["opaque"], outs["opaque swapped"])
    assert not np.array_equal(outs["translucent"], outs["translucent swapped"])
    dgs.close()


# ---- 2. white on transparent is the coverage of a plain text plan, on the GPU itself ---------------------------------
def _loads(font, c):
    """the font loader takes the character's glyph (it refuses what the reference panics on)"""
    try:
        font.glyph_by_index(font.glyph_index(ord(c)))
        return True
    except fr.FrError:
        return False


@pytest.mark.parametrize("name", ["DejaVuSans.ttf", "DejaVuSerif-Italic.ttf"])
def test_white_on_transparent_is_the_text_plan_coverage(ctx, name):
    import torch
    font = load_font(name, allow_hinted=True)
    whole = "".join(chr(c) for c in range(0x21, 0x7f)) + "".join(chr(c) for c in range(0xa1, 0x180))
    whole = "".join(c for c in whole if font.glyph_index(ord(c)) and _loads(font, c))
    gs, places, runs, shape = tw.lines(font, [whole[:120], whole[120:]], 18, pad=1)
    dgs = fr.DeviceGlyphSet(ctx, gs)
    white = np.full((len(places), 4), 255, np.uint8)
    for n, center, flags in CONFIGS:
        got = G.render_rgba(ctx, dgs, places, white, runs, [(0, 0, 0, 0)] * len(runs), G.sent4(shape, SENT), n, center, flags)
        plan = fr.TextPlan(dgs, places, runs, fr.FR_COVERAGE_U8, n, G.phase(center), flags)
        cov = torch.full(shape, 0x5b, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        plan.render(cov.data_ptr(), shape[1], shape[0])
        ctx.sync()
        plan.close()
        cov = cov.cpu().numpy()
        inside = G.inside(runs, shape)
        for ch in range(4):
            assert np.array_equal(got[..., ch][inside], cov[inside]), (name, n, center, flags, ch)
        assert (cov[inside] > 0).sum() > 1000
    dgs.close()


# ---- 3. every sub-pixel pen --------------------------------------------------------------------------------------------
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
    dgs = fr.DeviceGlyphSet(ctx, gs)
    for n, center in [(4, True), (1, False), (2, True)]:
        got = G.render_rgba(ctx, dgs, places, cols, runs, clears, G.sent4(shape, SENT), n, center)
        assert np.array_equal(got, G.twin_rgba("plain", gs, places, cols, runs, clears, G.sent4(shape, SENT), n, center)), (n, center)
        G.check_borders(got, runs, SENT)
    dgs.close()


# ---- 4. clipping at run borders, several runs with different clear colours --------------------------------------------
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
    rng = np.random.default_rng(5)
    clears = [tuple(int(v) for v in rng.integers(0, 256, 4)) for _ in range(len(runs))]
    shape = (2 + 5 * (H + 3) + 14, 8 * (W + 4) + 9)
    dgs = fr.DeviceGlyphSet(ctx, gs)
    for cols in (np.array([PINK] * len(rows), np.uint8), rng.integers(0, 256, (len(rows), 4)).astype(np.uint8)):
        got = G.render_rgba(ctx, dgs, places, cols, runs, clears, G.sent4(shape, SENT))
        assert np.array_equal(got, G.twin_rgba("plain", gs, places, cols, runs, clears, G.sent4(shape, SENT)))
        G.check_borders(got, runs, SENT)
        last = runs[-1]
        assert (got[last["out_y"]:last["out_y"] + last["h"], last["out_x"]:last["out_x"] + last["w"]] == clears[-1]).all()
    dgs.close()


# ---- 5. glyphs the fast kernels do not take -----------------------------------------------------------------------------
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
    dgs = fr.DeviceGlyphSet(ctx, gs)
    info = {}
    got = G.render_rgba(ctx, dgs, places, cols, runs, clears, G.sent4(shape, SENT), 4, True, info=info)
    assert info["stats"] == {"jobs_cov4": 0, "jobs_general": 4}, info
    assert info["pixels"] == sum(int(r["w"]) * int(r["h"]) for r in runs)
    assert "fr::text_rgba_kernel<4, 0, 1> x" in info["describe"], info
    assert np.array_equal(got, G.twin_rgba("plain", gs, places, cols, runs, clears, G.sent4(shape, SENT), 4, True))
    got = G.render_rgba(ctx, dgs, places, cols, runs, clears, G.sent4(shape, SENT), 2, False, FILL, info=info)
    assert "fr::text_rgba_kernel<2, 1, 1> x" in info["describe"], info
    assert np.array_equal(got, G.twin_rgba("plain", gs, places, cols, runs, clears, G.sent4(shape, SENT), 2, False, FILL))
    dgs.close()


# ---- 6. thousands of runs, and the graph / overlap options ---------------------------------------------------------------
def test_many_runs_graph_and_overlap(ctx):
    font = load_font("DejaVuSerif-Italic.ttf")
    rng = np.random.default_rng(2025)
    alphabet = np.array(list("abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789ffjT.,;!? "))
    strings = ["".join(rng.choice(alphabet, int(rng.integers(3, 24)))) for _ in range(2500)]
    gs, places, runs, (H, W) = tw.lines(font, strings, 14, pad=1)
    half = len(runs) // 2
    y_off = int(runs[half]["out_y"]) - 1
    runs["out_x"][half:] += W
    runs["out_y"][half:] -= y_off
    shape = (max(H - y_off, int(runs["out_y"][half - 1] + runs["h"][half - 1] + 1)), 2 * W)
    cols = _alternating(strings, PINK, (40, 200, 90, 255))
    cols[len(cols) // 2:, 3] = 150                                    # translucent in the second half
    clears = [(0, 0, 0, 0) if r % 2 else (250, 250, 250, 255) for r in range(len(runs))]
    dgs = fr.DeviceGlyphSet(ctx, gs)
    base = G.render_rgba(ctx, dgs, places, cols, runs, clears, G.sent4(shape, SENT))
    G.check_borders(base, runs, SENT)
    which = sorted(rng.choice(len(runs), 40, replace=False).tolist()) + [half - 1, half, len(runs) - 1]
    want = G.twin_rgba("plain", gs, places, cols, runs, clears, G.sent4(shape, SENT), which=which)
    for r in which:
        run = runs[r]
        sl = np.s_[run["out_y"]:run["out_y"] + run["h"], run["out_x"]:run["out_x"] + run["w"]]
        assert np.array_equal(base[sl], want[sl]), r
    try:
        ctx.set_option("graph", 1)
        for _ in range(3):
            assert np.array_equal(G.render_rgba(ctx, dgs, places, cols, runs, clears, G.sent4(shape, SENT)), base)
        ctx.set_option("graph", 0)
        for ov in (0, 2):
            ctx.set_option("overlap", ov)
            assert np.array_equal(G.render_rgba(ctx, dgs, places, cols, runs, clears, G.sent4(shape, SENT)), base)
    finally:
        ctx.set_option("graph", 0)
        ctx.set_option("overlap", 1)
    dgs.close()


# ---- 7. describe, and validation --------------------------------------------------------------------------------------------
def test_describe_and_validation_errors(ctx):
    font = load_font("DejaVuSans.ttf", allow_hinted=True)
    gs, _ = font.glyphset([font.glyph_index(ord("A")), font.glyph_index(ord("B"))], skip_unsupported=False)
    dgs = fr.DeviceGlyphSet(ctx, gs)
    s = np.float32(20) / np.float32(2048)
    places = rg.make_places([(0, 64, 16), (1, 700, 16)])
    runs = rg.make_runs([(0, 2, 30, 20, 0, 0, s)])
    cols, clears = np.array([PINK, PINK], np.uint8), np.zeros((1, 4), np.uint8)
    try:                        # (a plan or glyph set left open when an assertion fails must not outlive the context)
        _describe_and_validate(ctx, ctx._lib, dgs, places, runs, cols, clears, s)
    finally:
        dgs.close()


def _describe_and_validate(ctx, lib, dgs, places, runs, cols, clears, s):
    with closing(fr.TextPlanRGBA(dgs, places, cols, runs, clears)) as plan:
        assert plan.describe() == "fr::prepare_kernel x2; fr::text_rgba_kernel<4, 0, 0> x2"
        assert plan.pixels == 600 and plan.stats() == {"jobs_cov4": 0, "jobs_general": 2}
    with closing(fr.TextPlanRGBA(dgs, places, np.array([PINK, (1, 2, 3, 254)], np.uint8), runs, clears, 2,
                                 fr.FR_SAMPLE_CORNER, FILL)) as plan:
        assert plan.describe() == "fr::prepare_fill_kernel x2; fr::text_rgba_kernel<2, 1, 1> x2"

    def code(pl=places, pc=cols, rn=runs, rc=clears, n_pl=None, n_rn=None, mode=fr.FR_COVERAGE_U8, n=4,
             phase=fr.FR_SAMPLE_CENTER, flags=0):
        params = fr._lib.RasterParams(mode, n, phase, 0)
        h = C.c_void_p()
        ptr = (lambda a: None if a is None else fr._lib.ptr(a))
        rc_ = lib.fr_text_plan_create_rgba(ctx._h, dgs._h, ptr(pl), ptr(pc), len(pl) if n_pl is None else n_pl, ptr(rn),
                                           ptr(rc), len(rn) if n_rn is None else n_rn, C.byref(params), flags, C.byref(h))
        if rc_ == 0:
            lib.fr_plan_destroy(h)
        return rc_

    assert code() == 0
    assert code(pc=None) == -1                                                  # NULL colours with places
    assert code(rc=None) == -1                                                  # NULL clear colours with runs
    assert code(pl=places[:0], pc=None, rn=runs[:0], rc=None) == 0             # NULL with zero counts is fine
    assert code(flags=2) == -1                                                  # unknown flag bits
    assert code(phase=2) == -1
    assert code(mode=9) == -1                                                   # unknown mode
    for mode, n in [(fr.FR_MASK_NONZERO, 1), (fr.FR_WINDING_I16, 1), (fr.FR_GRAY_DEBUG, 1), (fr.FR_SDF_U8, 1),
                    (fr.FR_COVERAGE_U8, 3), (fr.FR_COVERAGE_U8, 8), (fr.FR_COVERAGE_U8, 0)]:
        assert code(mode=mode, n=n) == -4, (mode, n)
    # the checks of fr_text_plan_create apply unchanged
    assert code(rn=rg.make_runs([(0, 1, 30, 20, 0, 0, s), (1, 1, 30, 20, 29, 19, s)]), rc=np.zeros((2, 4), np.uint8)) == -1
    assert code(pl=rg.make_places([(0, 64, 16), (2, 700, 16)])) == -1          # glyph index out of range
    assert code(rn=rg.make_runs([(1, 2, 30, 20, 0, 0, s)])) == -1             # places beyond the table
    assert code(rn=rg.make_runs([(0, 2, 30, 20, 0, 0, 0.0)])) == -1            # scale must be > 0
    assert code(rn=rg.make_runs([(0, 2, 30, 20, 0, 0, 2.0 ** -21)])) == -4     # scale outside [2^-20, 2^20]
    assert code(rn=rg.make_runs([(0, 2, 70000, 20, 0, 0, s)])) == -4           # run larger than 65535
    assert code(pl=rg.make_places([(0, 64 << 23, 16), (1, 700, 16)])) == -4    # pen beyond 2^22 pixels
    with pytest.raises(ValueError):
        fr.TextPlanRGBA(dgs, places, cols[:1], runs, clears)
    # render-time: too small, a pitch beyond 2^26 pixels, an output not 4-byte aligned — the buffer is left untouched
    with closing(fr.TextPlanRGBA(dgs, places, cols, runs, clears)) as plan:
        _render_time_errors(ctx, plan)


def _render_time_errors(ctx, plan):
    import torch
    buf = torch.from_numpy(np.tile(SENT, (21, 31, 1))).to("cuda:0")
    torch.cuda.synchronize()
    for ptr, stride, rows in [(buf.data_ptr(), 29, 20), (buf.data_ptr(), (1 << 26) + 1, 20), (buf.data_ptr() + 2, 30, 20),
                              (buf.data_ptr() + 1, 30, 20)]:
        with pytest.raises(fr.FrError) as e:
            plan.render(ptr, stride, rows)
        assert e.value.code == -1, (ptr - buf.data_ptr(), stride)
    ctx.sync()
    assert (buf.cpu().numpy() == SENT).all()
    plan.render(buf.data_ptr() + 4 * 32, 31, 20)                          # aligned, one row and one pixel in: fine
    ctx.sync()
    got = buf.cpu().numpy()
    assert (got[0] == SENT).all() and (got[1:, 0] == SENT).all() and not (got[1:, 1:] == SENT).all(axis=2).any()


# ---- 8. the Python path: render_text_rgba -> qoi.saveRGBA -> Pillow ----------------------------------------------------------
def test_render_text_rgba_saves_as_qoi(ctx):
    from PIL import Image
    from font_renderer_amd import qoi
    font = load_font("DejaVuSerif-Italic.ttf")
    text = "Tffj a red word"
    im = fr.render_text_rgba(font, text, 27, ctx=ctx)
    gs, places, runs, shape = tw.lines(font, [text], 27)
    assert (im.height, im.width) == shape
    cols = np.array([(225, 105, 180, 255)] * len(text), np.uint8)
    assert np.array_equal(im.as_3d(), tw.rgba_render_run("plain", gs, places, cols, runs[0], (0, 0, 0, 0), None, 4, True))
    # RGB premultiplied by the coverage: white on transparent would be the coverage byte in every channel
    cov = fr.render_text(font, text, 27, ctx=ctx).as_2d()
    assert np.array_equal(im.as_3d()[..., 3], cov)
    back = np.asarray(Image.open(io.BytesIO(qoi.saveRGBA(im))).convert("RGBA"))
    assert np.array_equal(back, im.as_3d())
    # a highlighted word on an opaque background
    hl = [(255, 0, 0, 255) if 6 <= k < 9 else (0, 0, 0, 255) for k in range(len(text))]
    im2 = fr.render_text_rgba(font, text, 27, background=(255, 255, 255, 255), colors=hl, samples_per_axis=2,
                              phase=fr.FR_SAMPLE_CORNER, ctx=ctx)
    want = tw.rgba_render_run("plain", gs, places, np.array(hl, np.uint8), runs[0], (255, 255, 255, 255), None, 2, False)
    assert np.array_equal(im2.as_3d(), want)
    assert (im2.as_3d()[..., 3] == 255).all() and (im2.as_3d()[..., 0] > im2.as_3d()[..., 1]).any()

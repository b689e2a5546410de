"""Text runs on the GPU (fr_text_plan_create, include/fr_raster.h): byte for byte against the CPU twin of the definition
(tests/text_twin.py) or, for whole-pixel single instances, against fr_render_batch of the equivalent job.  Outputs are
sentinel-filled device buffers: bytes outside every run must keep the sentinel."""
import numpy as np
import pytest

import font_renderer_amd as fr
import text_gpu as G
import text_twin as tw
from fixtures import load_font
from font_renderer_amd import render_glyph as rg
from font_renderer_amd.glyph import GlyphSet
from font_renderer_amd.synth import synth_glyphset
from text_gpu import FILL

pytestmark = pytest.mark.gpu
SENT = 0x5b


# ---- 1. one whole-pixel instance is the ordinary job ----------------------------------------------------------------
@pytest.mark.parametrize("font_size", [13, 32])
def test_one_instance_equals_the_job(ctx, ascii_set, font_size):
    gs = ascii_set.gs
    cells = []
    for g in range(len(ascii_set)):
        scale = np.float32(font_size) / np.float32(int(ascii_set.g_upm[g]))
        c0, r0, w, h = tw.plain_cell(gs.boxes[g], scale, 0, 0)
        cells.append((c0, -r0, w, h, scale))
    CW, CH, cols = max(c[2] for c in cells) + 3, max(c[3] for c in cells) + 3, 24
    shape = (CH * ((len(cells) + cols - 1) // cols), CW * cols)
    places = rg.make_places([(g, -64 * c[0], c[1]) for g, c in enumerate(cells)])
    runs = rg.make_runs([(g, 1, c[2], c[3], (g % cols) * CW + 1, (g // cols) * CH + 2, c[4]) for g, c in enumerate(cells)])
    jobs = rg.make_jobs([(g, c[0], c[1], c[2], c[3], (g % cols) * CW + 1, (g // cols) * CH + 2, c[4]) for g, c in enumerate(cells)])
    dgs = fr.DeviceGlyphSet(ctx, gs)
    for mode, n in [(fr.FR_MASK_NONZERO, 1), (fr.FR_COVERAGE_U8, 1), (fr.FR_COVERAGE_U8, 2), (fr.FR_COVERAGE_U8, 4)]:
        for center in (False, True):
            for flags in (0, FILL):
                got = G.render_gray(ctx, dgs, places, runs, shape, mode, n, center, flags)
                want = np.full(shape, SENT, np.uint8)
                rg.render_batch(dgs, jobs, mode, want, n, G.phase(center), flags)
                assert np.array_equal(got, want), (font_size, mode, n, center, flags)
    dgs.close()


# ---- 2. real strings, overlapping instances, fractional pens --------------------------------------------------------
STRINGS = ["ffi fj Tf ff", "Tjfyfgf jjj", "Wavy /// fff", "ƒ∫ fî T,"]


@pytest.mark.parametrize("font_size,n,center", [(16, 4, True), (23, 2, False), (40, 1, True), (11, 4, False)])
def test_overlapping_strings_equal_the_twin(ctx, font_size, n, center):
    font = load_font("DejaVuSerif-Italic.ttf")
    gs, places, runs, shape = tw.lines(font, STRINGS, font_size, pad=2)
    assert any(p % 64 for p in places["pen_x64"]), "the pens must have fractional parts"
    dgs = fr.DeviceGlyphSet(ctx, gs)
    for flags in (0, FILL):
        got = G.render_gray(ctx, dgs, places, runs, shape, fr.FR_COVERAGE_U8, n, center, flags)
        assert np.array_equal(got, G.twin_gray("plain", gs, places, runs, shape, n, center, flags == FILL)), (font_size, n, flags)
    dgs.close()
    # instances of different glyphs share pixels, and the union is not the max of the separate coverages
    overlaps, differs = 0, 0
    for r in range(len(runs)):
        run = runs[r]
        sep = []
        for k in range(int(run["first"]), int(run["first"]) + int(run["count"])):
            one = run.copy()
            one["first"], one["count"] = k, 1
            sep.append(tw.render_run("plain", gs, places, one, n, center))
        cov = np.stack(sep)
        overlaps += int(((cov > 0).sum(0) > 1).sum())
        differs += int((cov.max(0) != tw.render_run("plain", gs, places, run, n, center)).sum())
    assert overlaps > 0
    if n > 1:
        assert differs > 0


def test_render_text_matches_the_twin(ctx):
    font = load_font("DejaVuSerif-Italic.ttf")
    for text, size in [("Tffj fix", 27), ("jump", 9)]:
        im = fr.render_text(font, text, size, ctx=ctx)
        gs, places, runs, shape = tw.lines(font, [text], size)
        assert (im.height, im.width) == shape
        assert np.array_equal(im.as_2d(), tw.render_run("plain", gs, places, runs[0], 4, True))


# ---- 3. every sub-pixel pen ------------------------------------------------------------------------------------------
def test_every_pen_fraction(ctx):
    font = load_font("DejaVuSans.ttf", allow_hinted=True)
    gs, kept = font.glyphset([font.glyph_index(ord("M")), font.glyph_index(ord("o"))], skip_unsupported=False)
    scale = np.float32(19) / np.float32(2048)
    W, H = 40, 30
    rows = []
    for g in range(2):
        for f in range(64):
            rows.append((g, 64 * 5 + f, 22))
            rows.append((g, 64 * 6 + f, 22))                       # the same pen one pixel to the right
    places = rg.make_places(rows)
    runs = rg.make_runs([(k, 1, W, H, (k % 16) * (W + 1), (k // 16) * (H + 1), scale) for k in range(len(rows))])
    shape = (16 * (H + 1), 16 * (W + 1))
    dgs = fr.DeviceGlyphSet(ctx, gs)
    for n, center in [(4, True), (1, False), (2, True)]:
        got = G.render_gray(ctx, dgs, places, runs, shape, fr.FR_COVERAGE_U8, n, center)
        assert np.array_equal(got, G.twin_gray("plain", gs, places, runs, shape, n, center)), (n, center)
        for k in range(0, len(rows), 2):
            a = got[runs[k]["out_y"]:runs[k]["out_y"] + H, runs[k]["out_x"]:runs[k]["out_x"] + W]
            b = got[runs[k + 1]["out_y"]:runs[k + 1]["out_y"] + H, runs[k + 1]["out_x"]:runs[k + 1]["out_x"] + W]
            assert np.array_equal(b[:, 1:], a[:, :-1]) and not b[:, 0].any(), (n, k)
    dgs.close()


# ---- 4. borders: the sentinel outside the runs, 0 outside the cells, clipping on every side --------------------------
def test_borders_and_clipping(ctx):
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
    # a run holding all four, and an empty run (no places) that must come out all 0
    rows += [(g, 200 + 640 * g // 2, 24) for g in range(4)]
    runs.append((k, 4, 60, 30, 3, 2 + 4 * (H + 3), scale))
    runs.append((0, 0, 11, 7, 70, 2 + 4 * (H + 3), scale))
    places, runs = rg.make_places(rows), rg.make_runs(runs)
    shape = (2 + 5 * (H + 3) + 14, 8 * (W + 4) + 9)
    dgs = fr.DeviceGlyphSet(ctx, gs)
    got = G.render_gray(ctx, dgs, places, runs, shape)
    want = G.twin_gray("plain", gs, places, runs, shape)
    assert np.array_equal(got, want)
    inside = np.zeros(shape, bool)
    for r in runs:
        inside[r["out_y"]:r["out_y"] + r["h"], r["out_x"]:r["out_x"] + r["w"]] = True
    assert (got[~inside] == SENT).all() and (got[inside] != SENT).any()
    last = runs[-1]
    assert not got[last["out_y"]:last["out_y"] + last["h"], last["out_x"]:last["out_x"] + last["w"]].any()
    # run pixels outside every cell are 0: the four-glyph run, right of its cells
    r4 = runs[-2]
    right = max(c[0] + c[2] for c in (tw.plain_cell(gs.boxes[int(p["glyph"])], scale, int(p["pen_x64"]), 24) for p in places[-4:]))
    assert right < int(r4["w"])
    assert not got[r4["out_y"]:r4["out_y"] + r4["h"], r4["out_x"] + right:r4["out_x"] + r4["w"]].any()
    dgs.close()


# ---- 5. glyphs the fast kernels do not take ------------------------------------------------------------------------
def test_large_glyph_and_tall_cell(ctx):
    big = synth_glyphset(1, 800, first_index=77)                       # > 768 segments
    font = load_font("DejaVuSans.ttf", allow_hinted=True)
    tall, _ = font.glyphset([font.glyph_index(ord("l")), font.glyph_index(ord("|"))], skip_unsupported=False)
    gs = GlyphSet([big.glyph(0), tall.glyph(0), tall.glyph(1)])
    s_big = np.float32(0.05)
    c0, r0, w0, h0 = tw.plain_cell(gs.boxes[0], s_big, 0, 0)
    s_tall = np.float32(700) / np.float32(2048)                          # 'l' at 700: > 512 rows, > 2048 sample rows at n = 4
    c1, r1, w1, h1 = tw.plain_cell(gs.boxes[1], s_tall, 0, 0)
    assert 4 * h1 > 2048
    places = rg.make_places([(0, -64 * c0 + 37, -r0), (0, -64 * c0 + 64 * 9 + 5, -r0 + 4),
                             (1, -64 * c1 + 21, -r1), (2, -64 * c1 + 64 * 30 + 50, -r1)])
    runs = rg.make_runs([(0, 2, w0 + 12, h0 + 5, 0, 0, s_big), (2, 2, 120, h1 + 1, w0 + 13, 0, s_tall)])
    shape = (max(h0 + 5, h1 + 1) + 1, w0 + 13 + 121)
    dgs = fr.DeviceGlyphSet(ctx, gs)
    info = {}
    got = G.render_gray(ctx, dgs, places, runs, shape, fr.FR_COVERAGE_U8, 4, True, info=info)
    assert info["stats"] == {"jobs_cov4": 0, "jobs_general": 4}, info
    assert info["pixels"] == sum(int(r["w"]) * int(r["h"]) for r in runs)
    assert "fr::text_kernel<4, 0>" in info["describe"], info
    assert np.array_equal(got, G.twin_gray("plain", gs, places, runs, shape, 4, True))
    got = G.render_gray(ctx, dgs, places, runs, shape, fr.FR_COVERAGE_U8, 2, False, FILL, info=info)
    assert "fr::text_kernel<2, 1>" in info["describe"], info
    assert np.array_equal(got, G.twin_gray("plain", gs, places, runs, shape, 2, False, True))
    dgs.close()


# ---- 6. thousands of runs, and the graph / overlap options -----------------------------------------------------------
def test_many_runs_graph_and_overlap(ctx):
    font = load_font("DejaVuSerif-Italic.ttf")
    rng = np.random.default_rng(2024)
    alphabet = np.array(list("abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789ffjT.,;!?"))
    strings = ["".join(rng.choice(alphabet, int(rng.integers(3, 24)))) for _ in range(2500)]
    gs, places, runs, (H, W) = tw.lines(font, strings, 14, pad=1)
    # two columns of runs, so the output is not one tall strip
    half = len(runs) // 2
    y_off = int(runs[half]["out_y"]) - 1
    runs["out_x"][half:] += W
    runs["out_y"][half:] -= y_off
    shape = (max(H - y_off, int(runs["out_y"][half - 1] + runs["h"][half - 1] + 1)), 2 * W)
    dgs = fr.DeviceGlyphSet(ctx, gs)
    base = G.render_gray(ctx, dgs, places, runs, shape)
    which = sorted(rng.choice(len(runs), 40, replace=False).tolist())
    want = G.twin_gray("plain", gs, places, runs, shape, which=which)
    for r in which:
        run = runs[r]
        sl = np.s_[run["out_y"]:run["out_y"] + run["h"], run["out_x"]:run["out_x"] + run["w"]]
        assert np.array_equal(base[sl], want[sl]), r
    try:
        ctx.set_option("graph", 1)
        for _ in range(2):
            assert np.array_equal(G.render_gray(ctx, dgs, places, runs, shape), base)
        ctx.set_option("graph", 0)
        ctx.set_option("overlap", 2)
        assert np.array_equal(G.render_gray(ctx, dgs, places, runs, shape), base)
    finally:
        ctx.set_option("graph", 0)
        ctx.set_option("overlap", 1)
    dgs.close()


# ---- 7. validation ---------------------------------------------------------------------------------------------------
def test_validation_errors(ctx):
    import torch
    font = load_font("DejaVuSans.ttf", allow_hinted=True)
    gs, _ = font.glyphset([font.glyph_index(ord("A")), font.glyph_index(ord("B"))], skip_unsupported=False)
    dgs = fr.DeviceGlyphSet(ctx, gs)
    s = np.float32(20) / np.float32(2048)
    places = rg.make_places([(0, 64, 16), (1, 700, 16)])
    runs = rg.make_runs([(0, 2, 30, 20, 0, 0, s)])

    def code(pl=places, rn=runs, mode=fr.FR_COVERAGE_U8, n=4, phase=fr.FR_SAMPLE_CENTER, flags=0):
        with pytest.raises(fr.FrError) as e:
            fr.TextPlan(dgs, pl, rn, mode, n, phase, flags)
        return e.value.code

    two = rg.make_runs([(0, 1, 30, 20, 0, 0, s), (1, 1, 30, 20, 29, 19, s)])
    assert code(rn=two) == -1                                                   # overlapping runs
    assert code(pl=rg.make_places([(0, 64, 16), (2, 700, 16)])) == -1          # glyph index out of range
    assert code(rn=rg.make_runs([(1, 2, 30, 20, 0, 0, s)])) == -1             # places beyond the table
    assert code(flags=2) == -1                                                  # unknown flag bits
    assert code(phase=2) == -1
    for mode, n in [(fr.FR_WINDING_I16, 1), (fr.FR_GRAY_DEBUG, 1), (fr.FR_SDF_U8, 1), (fr.FR_COVERAGE_U8, 3),
                    (fr.FR_COVERAGE_U8, 8), (fr.FR_MASK_NONZERO, 2)]:
        assert code(mode=mode, n=n) == -4, (mode, n)
    assert code(rn=rg.make_runs([(0, 2, 30, 20, 0, 0, 0.0)])) == -1            # scale must be > 0
    assert code(rn=rg.make_runs([(0, 2, 30, 20, 0, 0, 2.0 ** -21)])) == -4     # scale outside [2^-20, 2^20]
    assert code(rn=rg.make_runs([(0, 2, 70000, 20, 0, 0, s)])) == -4           # run larger than 65535
    assert code(pl=rg.make_places([(0, 64 << 23, 16), (1, 700, 16)])) == -4    # pen beyond 2^22 pixels
    # side by side and touching is not overlapping
    fr.TextPlan(dgs, places, rg.make_runs([(0, 1, 30, 20, 0, 0, s), (1, 1, 30, 20, 30, 0, s)])).close()
    # render-time: an output too small, a row pitch beyond 2^26 — the buffer is left untouched
    plan = fr.TextPlan(dgs, places, runs)
    buf = torch.full((20, 29), SENT, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    with pytest.raises(fr.FrError) as e:
        plan.render(buf.data_ptr(), 29, 20)
    assert e.value.code == -1
    with pytest.raises(fr.FrError) as e:
        plan.render(buf.data_ptr(), (1 << 26) + 1, 20)
    assert e.value.code == -1
    ctx.sync()
    assert (buf.cpu().numpy() == SENT).all()
    plan.close()
    dgs.close()

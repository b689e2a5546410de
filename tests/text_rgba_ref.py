"""CPU twin of RGBA text plans (include/fr_raster.h), written from the definition and not from the
kernel: the cells, clipping and sample points of tests/text_ref.py and the reference's winding (ref_numpy.winding_at) or
FR_FILL_CONSISTENT's (fill_rule_ref.winding_fill) per instance, kept PER INSTANCE, not as a union.  Every sub-sample of a
run starts at its clear colour; the instances are applied in placement order, each to the samples where its winding is
non-zero, by c' = (C.c * A + c * (255 - A) + 127) div 255 for R G B and a' = A; each channel of a pixel is then
(sum of its n x n samples + n^2 / 2) div n^2."""
import numpy as np

import fill_rule_ref
import ref_numpy
import text_ref

F = np.float32


def instance_hits(gs, places, run, n=1, center=False, fill=False):
    """-> [(k, y0, x0, hit)] in placement order: hit is the (rows n, cols n) bool non-zero test of instance k over its
    clipped cell, whose top-left pixel is (y0, x0) of the run"""
    w, h, scale = int(run["w"]), int(run["h"]), F(run["scale"])
    ph = 0.5 if center else 0.0
    off = np.array([(k + ph) / n for k in range(n)], F)
    out = []
    for k in range(int(run["first"]), int(run["first"]) + int(run["count"])):
        g, pen_x64, pen_y = int(places[k]["glyph"]), int(places[k]["pen_x64"]), int(places[k]["pen_y"])
        pts, cs = text_ref.glyph_arrays(gs, g)
        if len(cs) < 2 or len(pts) == 0:
            continue
        c0, r0, cw, ch = text_ref.cell(gs.boxes[g], scale, pen_x64, pen_y)
        x0, x1, y0, y1 = max(c0, 0), min(c0 + cw, w), max(r0, 0), min(r0 + ch, h)
        if x0 >= x1 or y0 >= y1:
            continue
        ix, fx = pen_x64 // 64, F((pen_x64 % 64) / 64)
        xs = (np.arange(x0, x1, dtype=np.int64) - ix).astype(F)
        ys = (pen_y - np.arange(y0, y1, dtype=np.int64)).astype(F)
        cx = ((xs[:, None] + (off - fx)[None, :]).reshape(-1) / scale).astype(F)
        cy = ((ys[:, None] - off[None, :]).reshape(-1) / scale).astype(F)
        if fill:
            wd = fill_rule_ref.winding_fill(pts, cs, cx[None, :], cy[:, None])
        else:
            wd = ref_numpy.winding_at(pts, cs, cx[None, :], cy[:, None])
        out.append((k, y0, x0, wd != 0))
    return out


def blend(dst, c):
    """the definition's update of RGBA samples dst (..., 4) int64 by the colour c = (R, G, B, A)"""
    a = int(c[3])
    out = np.empty_like(dst)
    for ch in range(3):
        out[..., ch] = (int(c[ch]) * a + dst[..., ch] * (255 - a) + 127) // 255
    out[..., 3] = a
    return out


def run_samples(gs, places, place_rgba, run, clear, n=1, center=False, fill=False):
    """-> (h n, w n, 4) int64: every sub-sample's RGBA after the run's instances, in placement order"""
    w, h = int(run["w"]), int(run["h"])
    smp = np.empty((h * n, w * n, 4), np.int64)
    smp[:] = np.asarray(clear, np.int64)
    for k, y0, x0, hit in instance_hits(gs, places, run, n, center, fill):
        view = smp[y0 * n:y0 * n + hit.shape[0], x0 * n:x0 * n + hit.shape[1]]
        view[hit] = blend(view[hit], place_rgba[k])
    return smp


def resolve(smp, n):
    """(sum over each pixel's n x n samples + n^2/2) div n^2 per channel -> (h, w, 4) u8"""
    h, w = smp.shape[0] // n, smp.shape[1] // n
    s = smp.reshape(h, n, w, n, 4).sum(axis=(1, 3))
    return ((s + n * n // 2) // (n * n)).astype(np.uint8)


def render_run(gs, places, place_rgba, run, clear, n=1, center=False, fill=False):
    return resolve(run_samples(gs, places, place_rgba, run, clear, n, center, fill), n)


def render_runs(gs, places, place_rgba, runs, run_clear, out, n=1, center=False, fill=False, which=None):
    """every run (or the runs `which`) into the (rows, cols, 4) u8 array `out`, as an RGBA text plan writes it"""
    for r in (range(len(runs)) if which is None else which):
        run = runs[r]
        img = render_run(gs, places, place_rgba, run, run_clear[r], n, center, fill)
        oy, ox = int(run["out_y"]), int(run["out_x"])
        out[oy:oy + img.shape[0], ox:ox + img.shape[1]] = img
    return out


def lines(font, strings, size, pad=0):
    """one run per string, stacked, laid out as tests/test_gpu_text.py lays them out: the run is the union of the string's
    instance cells, `pad` pixels between runs -> (glyph set, places, runs, (rows, cols))"""
    from font_renderer_amd import render_glyph as rg
    lay = [font.layout(s, size) for s in strings]
    distinct = sorted({int(g) for gi, _, _ in lay for g in gi})
    gs, kept = font.glyphset(distinct, skip_unsupported=False)
    local = {g: k for k, g in enumerate(kept)}
    scale = np.float32(size) / np.float32(font.information.units_per_em)
    seg = gs.segments_per_glyph()
    places, runs, y, W = [], [], pad, 0
    for gi, pen, _ in lay:
        cells = [text_ref.cell(gs.boxes[local[int(g)]], scale, int(p), 0) for g, p in zip(gi, pen) if seg[local[int(g)]]]
        left, top = min(c[0] for c in cells), min(c[1] for c in cells)
        shift = max(-left, 0)
        w = max(c[0] + c[2] for c in cells) + shift
        h = max(c[1] + c[3] for c in cells) - top
        runs.append((len(places), len(gi), w, h, pad, y, scale))
        places += [(local[int(g)], int(p) + 64 * shift, -top) for g, p in zip(gi, pen)]
        y += h + pad
        W = max(W, w + 2 * pad)
    return gs, rg.make_places(places), rg.make_runs(runs), (y, W)

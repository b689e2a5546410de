"""CPU twin of text plans of fr_glyph_place_ex placements (fr_text_plan_create_ex / fr_text_plan_create_rgba_ex,
include/fr_raster.h), written from the definition and not from the kernels, in numpy binary32 with
one rounding per written operation: per placement its own scale s (0: the run's), slant k and a pen kept to 1/64 pixel
in both axes; the cell of the sheared box, one column / row wider when the pen has a fractional part, clipped to the
run; the sample map
    cy = (f32(iy - Y) + (fy - off(j))) / s,   t = (f32(X - ix) + (off(i) - fx)) / s,   cx = t - k * cy
so that cx is a 2-D array (sample rows x sample columns); the reference's winding (ref_numpy.winding_at) or
FR_FILL_CONSISTENT's (fill_rule_ref.winding_fill) per instance.  Colour is not restated here: blend and resolve are
those of tests/text_rgba_ref.py and tests/text_srgb_ref.py, and the samples' start values (the run's clear colour, or
for FR_TEXT_LOAD the pixels already there) are what those twins and tests/text_load_ref.py start from."""
import math

import numpy as np

import fill_rule_ref
import ref_numpy
import text_load_ref as tl
import text_ref
import text_rgba_ref as tr
import text_srgb_ref as ts

F = np.float32


def place_params(pl, run):
    """-> (glyph, pen_x64, pen_y64, s, k) of one fr_glyph_place_ex in its run"""
    s = F(pl["scale"])
    return int(pl["glyph"]), int(pl["pen_x64"]), int(pl["pen_y64"]), (s if s != 0 else F(run["scale"])), F(pl["slant"])


def cell(box, s, k, pen_x64, pen_y64, widen=0):
    """(column 0, row 0, width, height) of an instance in image coordinates, before clipping; widen: that many more
    columns on each side (only to test that the cell holds the glyph)"""
    s, k = F(s), F(k)
    x_min, y_min, x_max, y_max = (F(int(v)) for v in box)
    lo = min(F(x_min + F(k * y_min)), F(x_min + F(k * y_max)))
    hi = max(F(x_max + F(k * y_min)), F(x_max + F(k * y_max)))
    mn_x, mx_x = math.floor(F(lo * s)), math.ceil(F(hi * s))
    mn_y, mx_y = math.floor(F(y_min * s)), math.ceil(F(y_max * s))
    ix, fx64, iy, fy64 = pen_x64 // 64, pen_x64 % 64, pen_y64 // 64, pen_y64 % 64
    return (ix + mn_x - widen, iy - mx_y, mx_x - mn_x + 1 + (1 if fx64 else 0) + 2 * widen,
            mx_y - mn_y + 1 + (1 if fy64 else 0))


def instance_hits(gs, places, run, n=1, center=False, fill=False, widen=0):
    """-> [(k, y0, x0, hit)] in placement order: hit is the (rows n, cols n) bool non-zero test of instance k over its
    clipped cell, whose top-left pixel is (y0, x0) of the run"""
    w, h = int(run["w"]), int(run["h"])
    ph = 0.5 if center else 0.0
    off = np.array([(q + ph) / n for q in range(n)], F)
    out = []
    for idx in range(int(run["first"]), int(run["first"]) + int(run["count"])):
        g, pen_x64, pen_y64, s, k = place_params(places[idx], run)
        pts, cs = text_ref.glyph_arrays(gs, g)
        if len(cs) < 2 or len(pts) == 0:
            continue
        c0, r0, cw, ch = cell(gs.boxes[g], s, k, pen_x64, pen_y64, widen)
        x0, x1, y0, y1 = max(c0, 0), min(c0 + cw, w), max(r0, 0), min(r0 + ch, h)
        if x0 >= x1 or y0 >= y1:
            continue
        ix, fx, iy, fy = pen_x64 // 64, F((pen_x64 % 64) / 64), pen_y64 // 64, F((pen_y64 % 64) / 64)
        xs = (np.arange(x0, x1, dtype=np.int64) - ix).astype(F)
        ys = (iy - np.arange(y0, y1, dtype=np.int64)).astype(F)
        t = ((xs[:, None] + (off - fx)[None, :]).reshape(-1) / s).astype(F)       # (off(i) - fx): exact
        cy = ((ys[:, None] + (fy - off)[None, :]).reshape(-1) / s).astype(F)      # (fy - off(j)): exact
        kcy = (k * cy).astype(F)
        cx = (t[None, :] - kcy[:, None]).astype(F)
        wind = fill_rule_ref.winding_fill if fill else ref_numpy.winding_at
        out.append((idx, y0, x0, wind(pts, cs, cx, cy[:, None]) != 0))
    return out


def run_samples(gs, places, run, n=1, center=False, fill=False, widen=0):
    """-> (h n, w n) bool: is some instance's winding non-zero at each sub-sample of the run"""
    hit = np.zeros((int(run["h"]) * n, int(run["w"]) * n), bool)
    for _, y0, x0, m in instance_hits(gs, places, run, n, center, fill, widen):
        hit[y0 * n:y0 * n + m.shape[0], x0 * n:x0 * n + m.shape[1]] |= m
    return hit


def render_run(gs, places, run, n=1, center=False, fill=False):
    return text_ref.to_bytes(run_samples(gs, places, run, n, center, fill), n)


def render_runs(gs, places, runs, out, n=1, center=False, fill=False, which=None):
    """every run (or the runs `which`) into `out`, as a text plan writes it"""
    for r in (range(len(runs)) if which is None else which):
        run = runs[r]
        img = render_run(gs, places, run, n, center, fill)
        oy, ox = int(run["out_y"]), int(run["out_x"])
        out[oy:oy + img.shape[0], ox:ox + img.shape[1]] = img
    return out


def _no_instances(run):
    """the run with no placement: the colour twins then return the samples' start values"""
    r0 = np.array(run).copy()
    r0["count"] = 0
    return r0


def rgba_run_samples(gs, places, place_rgba, run, clear=None, dst=None, n=1, center=False, fill=False, srgb=False):
    """-> (h n, w n, 4) int64: every sub-sample's RGBA after the run's instances, in placement order.  The samples start
    at `clear`, or (FR_TEXT_LOAD) at the run's (h, w, 4) pixels `dst`, R G B A"""
    if dst is not None:
        smp = tl.run_samples(gs, None, None, _no_instances(run), dst, n, center, fill, srgb)
    else:
        smp = (ts if srgb else tr).run_samples(gs, None, None, _no_instances(run), clear, n, center, fill)
    blend = ts.blend if srgb else tr.blend
    for k, y0, x0, hit in instance_hits(gs, places, run, n, center, fill):
        view = smp[y0 * n:y0 * n + hit.shape[0], x0 * n:x0 * n + hit.shape[1]]
        view[hit] = blend(view[hit], place_rgba[k])
    return smp


def rgba_render_run(gs, places, place_rgba, run, clear=None, dst=None, n=1, center=False, fill=False, srgb=False, bgr=False):
    """the run's (h, w, 4) u8 pixels in the stored byte order (dst, if given, is in that order too)"""
    if dst is not None and bgr:
        dst = ts.bgra(dst)
    smp = rgba_run_samples(gs, places, place_rgba, run, clear, dst, n, center, fill, srgb)
    img = ts.resolve(smp, n) if srgb else tr.resolve(smp, n)
    return ts.bgra(img) if bgr else img


def rgba_render_runs(gs, places, place_rgba, runs, run_clear, out, n=1, center=False, fill=False, srgb=False, bgr=False,
                     load=False, which=None):
    """every run (or the runs `which`) into the (rows, cols, 4) u8 array `out`, in place, as the plan writes it; load:
    drawn over what `out` holds (run_clear is then ignored)"""
    for r in (range(len(runs)) if which is None else which):
        run = runs[r]
        oy, ox, h, w = int(run["out_y"]), int(run["out_x"]), int(run["h"]), int(run["w"])
        if not w or not h:
            continue
        sl = np.s_[oy:oy + h, ox:ox + w]
        out[sl] = rgba_render_run(gs, places, place_rgba, run, None if load else run_clear[r], out[sl].copy() if load else None,
                                  n, center, fill, srgb, bgr)
    return out


def met_tiles(gs, places, runs, tile_w=64, tile_h=16):
    """the 64 x 16 tiles of the runs that some clipped instance cell meets -> set of (run, tile row, tile column)"""
    met = set()
    for r in range(len(runs)):
        run = runs[r]
        w, h = int(run["w"]), int(run["h"])
        for idx in range(int(run["first"]), int(run["first"]) + int(run["count"])):
            g, pen_x64, pen_y64, s, k = place_params(places[idx], run)
            pts, cs = text_ref.glyph_arrays(gs, g)
            if len(cs) < 2 or len(pts) == 0:
                continue
            c0, r0, cw, ch = cell(gs.boxes[g], s, k, pen_x64, pen_y64)
            x0, x1, y0, y1 = max(c0, 0), min(c0 + cw, w), max(r0, 0), min(r0 + ch, h)
            if x0 >= x1 or y0 >= y1:
                continue
            met |= {(r, ty, tx) for ty in range(y0 // tile_h, (y1 - 1) // tile_h + 1)
                    for tx in range(x0 // tile_w, (x1 - 1) // tile_w + 1)}
    return met

"""CPU twin of text plans of fr_glyph_place_affine placements (fr_text_plan_create_affine / fr_text_plan_create_rgba_affine,
include/fr_raster.h), written from the header and not from the kernel, in numpy binary32 with one
rounding per written operation; only the inverse matrix is binary64, as the header has it:
    D = f64(xx * yy) - f64(xy * yx),   q00 = f32(yy / D), q01 = f32(-xy / D), q10 = f32(-yx / D), q11 = f32(xx / D)
    dx = f32(X - ix) + (off(i) - fx),  dy = f32(iy - Y) + (fy - off(j))
    cx = f32(q00 * dx) + f32(q01 * dy),   cy = f32(q10 * dx) + f32(q11 * dy)
so that cx and cy are both 2-D arrays (sample rows x sample columns); the cell is that of the box's four mapped corners,
one column / row wider when the pen has a fractional part, clipped to the run; the winding is the reference's
(ref_numpy.winding_at) or FR_FILL_CONSISTENT's (fill_rule_ref.winding_fill) per instance.  Colour is not restated here:
blend, resolve and the samples' start values come through the functions tests/text_place_ref.py uses."""
import math

import numpy as np

import fill_rule_ref
import ref_numpy
import text_place_ref as tp
import text_ref
import text_rgba_ref as tr
import text_srgb_ref as ts

F = np.float32
D64 = np.float64


def inverse(m):
    """(q00, q01, q10, q11) as binary32 values, from the four binary32 entries of m in binary64"""
    xx, xy, yx, yy = (D64(F(v)) for v in m)
    det = D64(D64(xx * yy) - D64(xy * yx))
    return F(yy / det), F(-xy / det), F(-yx / det), F(xx / det)


def place_params(pl):
    """-> (glyph, pen_x64, pen_y64, m) of one fr_glyph_place_affine"""
    return int(pl["glyph"]), int(pl["pen_x64"]), int(pl["pen_y64"]), tuple(F(v) for v in pl["m"])


def cell(box, m, pen_x64, pen_y64, widen=0):
    """(column 0, row 0, width, height) of an instance in image coordinates, before clipping; widen: that many more
    pixels on every side (only to test that the cell holds the glyph)"""
    xx, xy, yx, yy = (F(v) for v in m)
    x_min, y_min, x_max, y_max = (F(int(v)) for v in box)
    corners = [(x, y) for x in (x_min, x_max) for y in (y_min, y_max)]
    u = [F(F(xx * x) + F(xy * y)) for x, y in corners]
    v = [F(F(yx * x) + F(yy * y)) for x, y in corners]
    mn_x, mx_x, mn_y, mx_y = math.floor(min(u)), math.ceil(max(u)), math.floor(min(v)), math.ceil(max(v))
    ix, fx64, iy, fy64 = pen_x64 // 64, pen_x64 % 64, pen_y64 // 64, pen_y64 % 64
    return (ix + mn_x - widen, iy - mx_y - widen, mx_x - mn_x + 1 + (1 if fx64 else 0) + 2 * widen,
            mx_y - mn_y + 1 + (1 if fy64 else 0) + 2 * widen)


def sample_coords(m, pen_x64, pen_y64, x0, x1, y0, y1, n=1, center=False):
    """(cx, cy), each ((y1 - y0) n, (x1 - x0) n) binary32, of the samples of image columns [x0, x1) and rows [y0, y1)"""
    q00, q01, q10, q11 = inverse(m)
    ph = 0.5 if center else 0.0
    off = np.array([(q + ph) / n for q in range(n)], F)
    ix, fx, iy, fy = pen_x64 // 64, F((pen_x64 % 64) / 64), pen_y64 // 64, F((pen_y64 % 64) / 64)
    xs = (np.arange(x0, x1, dtype=np.int64) - ix).astype(F)
    ys = (iy - np.arange(y0, y1, dtype=np.int64)).astype(F)
    dx = (xs[:, None] + (off - fx)[None, :]).reshape(-1).astype(F)            # (off(i) - fx): exact
    dy = (ys[:, None] + (fy - off)[None, :]).reshape(-1).astype(F)            # (fy - off(j)): exact
    cx = ((q00 * dx).astype(F)[None, :] + (q01 * dy).astype(F)[:, None]).astype(F)
    cy = ((q10 * dx).astype(F)[None, :] + (q11 * dy).astype(F)[:, None]).astype(F)
    return cx, cy


def instance_hits(gs, places, run, n=1, center=False, fill=False, widen=0):
    """-> [(k, y0, x0, hit)] in placement order: hit is the (rows n, cols n) bool non-zero test of instance k over its
    clipped cell, whose top-left pixel is (y0, x0) of the run.  widen: the cell that much larger on every side, unclipped
    (y0 and x0 may then be negative)"""
    w, h = int(run["w"]), int(run["h"])
    wind = fill_rule_ref.winding_fill if fill else ref_numpy.winding_at
    out = []
    for idx in range(int(run["first"]), int(run["first"]) + int(run["count"])):
        g, pen_x64, pen_y64, m = place_params(places[idx])
        pts, cs = text_ref.glyph_arrays(gs, g)
        if len(cs) < 2 or len(pts) == 0:
            continue
        c0, r0, cw, ch = cell(gs.boxes[g], m, pen_x64, pen_y64, widen)
        if widen:
            x0, x1, y0, y1 = c0, c0 + cw, r0, r0 + ch
        else:
            x0, x1, y0, y1 = max(c0, 0), min(c0 + cw, w), max(r0, 0), min(r0 + ch, h)
        if x0 >= x1 or y0 >= y1:
            continue
        cx, cy = sample_coords(m, pen_x64, pen_y64, x0, x1, y0, y1, n, center)
        out.append((idx, y0, x0, wind(pts, cs, cx, cy) != 0))
    return out


def run_samples(gs, places, run, n=1, center=False, fill=False):
    """-> (h n, w n) bool: is some instance's winding non-zero at each sub-sample of the run"""
    hit = np.zeros((int(run["h"]) * n, int(run["w"]) * n), bool)
    for _, y0, x0, m in instance_hits(gs, places, run, n, center, fill):
        hit[y0 * n:y0 * n + m.shape[0], x0 * n:x0 * n + m.shape[1]] |= m
    return hit


def render_run(gs, places, run, n=1, center=False, fill=False):
    return text_ref.to_bytes(run_samples(gs, places, run, n, center, fill), n)


def render_runs(gs, places, runs, out, n=1, center=False, fill=False):
    """every run into `out`, as a text plan writes it"""
    for run in runs:
        img = render_run(gs, places, run, n, center, fill)
        oy, ox = int(run["out_y"]), int(run["out_x"])
        out[oy:oy + img.shape[0], ox:ox + img.shape[1]] = img
    return out


def rgba_run_samples(gs, places, place_rgba, run, clear=None, dst=None, n=1, center=False, fill=False, srgb=False):
    """-> (h n, w n, 4) int64: every sub-sample's RGBA after the run's instances, in placement order; start values and
    blend as tests/text_place_ref.py::rgba_run_samples"""
    smp = tp.rgba_run_samples(gs, None, None, tp._no_instances(run), clear, dst, n, center, fill, srgb)
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
                     load=False):
    """every run into the (rows, cols, 4) u8 array `out`, in place, as the plan writes it; load: drawn over what `out`
    holds (run_clear is then ignored)"""
    for r, run in enumerate(runs):
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
    for r, run in enumerate(runs):
        w, h = int(run["w"]), int(run["h"])
        for idx in range(int(run["first"]), int(run["first"]) + int(run["count"])):
            g, pen_x64, pen_y64, m = place_params(places[idx])
            pts, cs = text_ref.glyph_arrays(gs, g)
            if len(cs) < 2 or len(pts) == 0:
                continue
            c0, r0, cw, ch = cell(gs.boxes[g], m, pen_x64, pen_y64)
            x0, x1, y0, y1 = max(c0, 0), min(c0 + cw, w), max(r0, 0), min(r0 + ch, h)
            if x0 >= x1 or y0 >= y1:
                continue
            met |= {(r, ty, tx) for ty in range(y0 // tile_h, (y1 - 1) // tile_h + 1)
                    for tx in range(x0 // tile_w, (x1 - 1) // tile_w + 1)}
    return met


def from_ex(places, runs):
    """fr_glyph_place_ex placements as fr_glyph_place_affine: m = {s, f32(s k), 0, s} with s the placement's (or its run's) scale"""
    from font_renderer_amd import render_glyph as rg
    rows = [None] * len(places)
    for run in runs:
        for idx in range(int(run["first"]), int(run["first"]) + int(run["count"])):
            g, px, py, s, k = tp.place_params(places[idx], run)
            rows[idx] = (g, px, py, F(s), F(F(s) * F(k)), F(0), F(s))
    return rg.make_places_affine(rows)

"""CPU twin of the text-run definition (include/fr_raster.h), written from the definition and not
from the kernels: each placement's cell (renderGlyph's grid at the run's scale, one column wider when the pen is
fractional) clipped to its run, the sample points with the sub-sample column offsets shifted by fx, the reference's
winding (ref_numpy.winding_at) or FR_FILL_CONSISTENT's (fill_rule_ref.winding_fill) per instance, and the union of the
non-zero tests over the instances, per sample."""
import math

import numpy as np

import fill_rule_ref
import ref_numpy

F = np.float32
MASK_NONZERO, COVERAGE_U8 = 2, 3


def glyph_arrays(gs, g):
    c0, c1 = int(gs.glyph_start[g]), int(gs.glyph_start[g + 1])
    p0 = int(gs.contour_start[c0])
    return gs.points_xy[p0:int(gs.contour_start[c1])], gs.contour_start[c0:c1 + 1] - np.uint32(p0)


def cell(box, scale, pen_x64, pen_y):
    """(column 0, row 0, width, height) of an instance in image coordinates, before clipping"""
    s = F(scale)
    b = [F(int(v)) * s for v in box]
    mn_x, mn_y, mx_x, mx_y = math.floor(b[0]), math.floor(b[1]), math.ceil(b[2]), math.ceil(b[3])
    ix, fx64 = pen_x64 // 64, pen_x64 % 64
    return ix + mn_x, pen_y - mx_y, mx_x - mn_x + 1 + (1 if fx64 else 0), mx_y - mn_y + 1


def run_samples(gs, places, run, n=1, center=False, fill=False):
    """-> (h n, w n) bool: is some instance's winding non-zero at each sub-sample of the run"""
    w, h, scale = int(run["w"]), int(run["h"]), F(run["scale"])
    hit = np.zeros((h * n, w * n), bool)
    ph = 0.5 if center else 0.0
    off = np.array([(k + ph) / n for k in range(n)], F)
    for k in range(int(run["first"]), int(run["first"]) + int(run["count"])):
        g, pen_x64, pen_y = int(places[k]["glyph"]), int(places[k]["pen_x64"]), int(places[k]["pen_y"])
        pts, cs = glyph_arrays(gs, g)
        if len(cs) < 2 or len(pts) == 0:
            continue
        c0, r0, cw, ch = cell(gs.boxes[g], scale, pen_x64, pen_y)
        x0, x1, y0, y1 = max(c0, 0), min(c0 + cw, w), max(r0, 0), min(r0 + ch, h)
        if x0 >= x1 or y0 >= y1:
            continue
        ix, fx = pen_x64 // 64, F((pen_x64 % 64) / 64)
        xs = (np.arange(x0, x1, dtype=np.int64) - ix).astype(F)
        ys = (pen_y - np.arange(y0, y1, dtype=np.int64)).astype(F)
        cx = ((xs[:, None] + (off - fx)[None, :]).reshape(-1) / scale).astype(F)        # (off(i) - fx): exact
        cy = ((ys[:, None] - off[None, :]).reshape(-1) / scale).astype(F)
        if fill:
            wd = fill_rule_ref.winding_fill(pts, cs, cx[None, :], cy[:, None])
        else:
            wd = ref_numpy.winding_at(pts, cs, cx[None, :], cy[:, None])
        hit[y0 * n:y1 * n, x0 * n:x1 * n] |= wd != 0
    return hit


def to_bytes(hit, n):
    """round_half_up(255 k / n^2) over each pixel's n x n sub-samples (n = 1: 255 / 0, FR_MASK_NONZERO's byte)"""
    h, w = hit.shape[0] // n, hit.shape[1] // n
    k = hit.reshape(h, n, w, n).sum(axis=(1, 3)).astype(np.int64)
    return ((510 * k + n * n) // (2 * n * n)).astype(np.uint8)


def render_run(gs, places, run, n=1, center=False, fill=False):
    return to_bytes(run_samples(gs, places, run, n, center, fill), n)


def render_runs(gs, places, runs, out, n=1, center=False, fill=False, which=None):
    """every run (or the runs `which`) into `out`, as a text plan writes it"""
    for r in (range(len(runs)) if which is None else which):
        run = runs[r]
        img = render_run(gs, places, run, n, center, fill)
        oy, ox = int(run["out_y"]), int(run["out_x"])
        out[oy:oy + img.shape[0], ox:ox + img.shape[1]] = img
    return out

"""Block glyphs (tests/text_block_cases.py) under fr_glyph_place_affine placements whose every number is exact: the
eight maps s * {quarter turns} and s * [[1, -1], [1, 1]] * {quarter turns} (45 degree steps), s in {1/4, 1/2, 1}, pens with
the fractions 0 and 37/64.  The inverse entries are then +-1/s or +-1/(2 s), every product and sum of the sample map
(include/fr_raster.h) is a multiple of 2^-12 below 2^12, hence a binary32 value, and the expected image comes from
Fractions alone: text_block_cases.crossings decides every sample, with that module's margin assert for the crossings
it cannot decide exactly.  Nothing here imports a float twin."""
import math
from fractions import Fraction as Fr
from functools import lru_cache

import numpy as np

import text_block_cases as bc
from font_renderer_amd import render_glyph as rg

SCALES = (Fr(1, 4), Fr(1, 2), Fr(1))
_R = (0, -1, 1, 0)                                        # a quarter turn counter-clockwise: (x, y) -> (-y, x)
_B = (1, -1, 1, 1)                                        # sqrt(2) times a turn of 45 degrees


def _mul(a, b):
    return (a[0] * b[0] + a[1] * b[2], a[0] * b[1] + a[1] * b[3], a[2] * b[0] + a[3] * b[2], a[2] * b[1] + a[3] * b[3])


def _turns(m):
    out = [m]
    for _ in range(3):
        out.append(_mul(out[-1], _R))
    return out


MAPS = _turns((1, 0, 0, 1)) + _turns(_B)                  # 0, 90, 180, 270 and 45, 135, 225, 315 degrees
assert MAPS[1] == (0, -1, 1, 0) and len(set(MAPS)) == 8


def _exact32(v):
    return bc._fits(v, 1 << 12)


def inverse(m):
    xx, xy, yx, yy = m
    det = xx * yy - xy * yx
    q = (yy / det, -xy / det, -yx / det, xx / det)
    assert det != 0 and all(bc.is_f32(v) for v in q + tuple(m))
    return q


def cell(box, m, pen_x64, pen_y64):
    """fr_glyph_place_affine's cell (column 0, row 0, width, height), unclipped"""
    xx, xy, yx, yy = m
    corners = [(x, y) for x in (box[0], box[2]) for y in (box[1], box[3])]
    u, v = [xx * x + xy * y for x, y in corners], [yx * x + yy * y for x, y in corners]
    assert all(_exact32(t) for t in u + v)
    mn_x, mx_x, mn_y, mx_y = math.floor(min(u)), math.ceil(max(u)), math.floor(min(v)), math.ceil(max(v))
    return ((pen_x64 // 64) + mn_x, (pen_y64 // 64) - mx_y, mx_x - mn_x + 1 + (1 if pen_x64 % 64 else 0),
            mx_y - mn_y + 1 + (1 if pen_y64 % 64 else 0))


def sample_coords(m, pen_x64, pen_y64, x0, x1, y0, y1, n, center):
    """exact (cx, cy) of every sample of image columns [x0, x1) and rows [y0, y1) -> two lists of rows of Fractions;
    asserts that every product and sum of the map is a binary32 value"""
    q00, q01, q10, q11 = inverse(m)
    ix, fx, iy, fy = pen_x64 // 64, Fr(pen_x64 % 64, 64), pen_y64 // 64, Fr(pen_y64 % 64, 64)
    off = bc.offs(n, center)
    dx = [(X - ix) + (o - fx) for X in range(x0, x1) for o in off]
    dy = [(iy - Y) + (fy - o) for Y in range(y0, y1) for o in off]
    ax, bx, ay, by = [q00 * d for d in dx], [q10 * d for d in dx], [q01 * d for d in dy], [q11 * d for d in dy]
    assert all(_exact32(v) for v in dx + dy + ax + bx + ay + by)
    cx = [[a + b for a in ax] for b in ay]
    cy = [[a + b for a in bx] for b in by]
    assert all(_exact32(v) for row in cx + cy for v in (min(row), max(row)))      # (multiples of 2^-12 between two such)
    return cx, cy


def exact_hits(g, cx, cy):
    """text_block_cases.winding_exact(g, cx, cy) != 0 for every sample (the crossings of each distinct height found once)
    -> bool array; asserts that module's margin condition"""
    pcs, cache = bc.pieces(g), {}
    out = np.zeros((len(cy), len(cy[0])), bool)
    for r in range(len(cy)):
        for c in range(len(cy[0])):
            y, x = cy[r][c], cx[r][c]
            cr = cache.get(y)
            if cr is None:
                cr = cache[y] = bc.crossings(g, y, pcs)
            w = 0
            for xx, sign, exact in cr:
                assert exact or abs(xx - x) >= bc.MARGIN, "%s: (%s, %s) is within 2^-6 of an inexact crossing" % (g.name, x, y)
                if xx >= x:
                    w += sign
            out[r, c] = w != 0
    return out


def place_of(pl):
    return int(pl["glyph"]), int(pl["pen_x64"]), int(pl["pen_y64"]), tuple(Fr(float(v)) for v in pl["m"])


def instance_hits(glyphs, places, run, n, center, widen=0):
    """-> [(placement index, y0, x0, hit, cx, cy)] over each instance's cell clipped to the run (widen: that many more
    pixels on every side, unclipped)"""
    out = []
    for idx in range(int(run["first"]), int(run["first"]) + int(run["count"])):
        gi, px, py, m = place_of(places[idx])
        g = glyphs[gi]
        c0, r0, cw, ch = cell(g.box, m, px, py)
        if widen:
            x0, x1, y0, y1 = c0 - widen, c0 + cw + widen, r0 - widen, r0 + ch + widen
        else:
            x0, x1, y0, y1 = max(c0, 0), min(c0 + cw, int(run["w"])), max(r0, 0), min(r0 + ch, int(run["h"]))
        if x0 >= x1 or y0 >= y1:
            continue
        cx, cy = sample_coords(m, px, py, x0, x1, y0, y1, n, center)
        out.append((idx, y0, x0, exact_hits(g, cx, cy), cx, cy))
    return out


def render_runs(glyphs, places, runs, out, n, center):
    """every run's exact coverage bytes into `out`, as a FR_FILL_CONSISTENT text plan must write them"""
    for run in runs:
        hit = np.zeros((int(run["h"]) * n, int(run["w"]) * n), bool)
        for _, y0, x0, m, _, _ in instance_hits(glyphs, places, run, n, center):
            hit[y0 * n:y0 * n + m.shape[0], x0 * n:x0 * n + m.shape[1]] |= m
        img = bc.coverage_bytes(hit, n)
        oy, ox = int(run["out_y"]), int(run["out_x"])
        out[oy:oy + img.shape[0], ox:ox + img.shape[1]] = img
    return out


def _ok(g, m, px, py, n, center):
    """does the margin condition hold on the placement's cell widened by one pixel: a condition of the exact geometry"""
    c0, r0, cw, ch = cell(g.box, m, px, py)
    try:
        exact_hits(g, *sample_coords(m, px, py, c0 - 1, c0 + cw + 1, r0 - 1, r0 + ch + 1, n, center))
    except AssertionError:
        return False
    return True


SLOT = 36                                                 # pixels per slot of the main run: 6 x 4 slots


@lru_cache(maxsize=None)
def block_case(n, center):
    """-> (glyphs, places, runs, shape).  Run 0, 216 x 144 at (3, 2): 24 placements, one per (map, scale), each in its own
    36 x 36 slot, so cells lie across the tile borders x = 64, 128 and y = 16, 32, ...; the pen fractions run through
    (0, 0), (37, 0), (0, 37), (37, 37).  The glyph is the curved "bump" where that placement keeps the margin condition
    and a line outline otherwise.  Run 1, 9 x 7 at (225, 5): the ring at 1/4 under the 45 degree map, clipped on all four
    sides.  Run 2, 70 x 20 at (5, 150): a square at every map around the corner (64, 16) of four tiles."""
    eg = {g.name: g for g in bc.edge_glyphs()}
    glyphs = [eg["two"], eg["stairs"], eg["notch"], eg["diamond"], eg["square"], eg["square5"],
              bc.BlockGlyph("slab", [bc.rect(0, 0, 12, 6)]), bc.cover(5, 1, 4), eg["bump"], eg["ring"]]
    by_scale = {Fr(1, 4): (0, 1, 2, 3), Fr(1, 2): (2, 3, 4, 5), Fr(1): (4, 6, 7, 5)}
    fracs = ((0, 0), (37, 0), (0, 37), (37, 37))
    rows, q = [], 0
    for si, s in enumerate(SCALES):
        for mi, mp in enumerate(MAPS):
            m = tuple(s * v for v in mp)
            fx, fy = fracs[(mi + si) % 4]
            gi = by_scale[s][(mi + si) % 4]
            if s < 1 and mi % 3 == 0 and _ok(glyphs[8], m, fx, fy, n, center):
                gi = 8
            c0, r0, cw, ch = cell(glyphs[gi].box, m, fx, fy)
            assert cw <= SLOT - 2 and ch <= SLOT - 2, (gi, mp, s, cw, ch)
            sx, sy = SLOT * (q % 6) + 1, SLOT * (q // 6) + 1
            rows.append((gi, fx + 64 * (sx - c0), fy + 64 * (sy - r0)) + tuple(float(v) for v in m))
            q += 1
    n_main = len(rows)
    m45 = tuple(Fr(1, 4) * v for v in MAPS[4])
    c0, r0, cw, ch = cell(glyphs[9].box, m45, 37, 0)
    rows.append((9, 37 + 64 * (-8 - c0), 64 * (-9 - r0)) + tuple(float(v) for v in m45))
    assert cw > 9 + 8 and ch > 7 + 9                      # the cell starts left of and above the run and ends beyond it
    first3 = len(rows)
    for mi, mp in enumerate(MAPS):
        m = tuple(Fr(1, 2) * v for v in mp)
        c0, r0, cw, ch = cell(glyphs[4].box, m, 0, 37)
        rows.append((4, 64 * (64 - 4 - c0), 37 + 64 * (16 - 5 - r0)) + tuple(float(v) for v in m))
        assert cw > 4 and ch > 5                          # every one of these cells holds pixel (64, 16) and (63, 15)
    runs = [(0, n_main, 6 * SLOT, 4 * SLOT, 3, 2, 1.0), (n_main, 1, 9, 7, 225, 5, 1.0), (first3, 8, 70, 20, 5, 150, 1.0)]
    return glyphs, rg.make_places_affine(rows), rg.make_runs(runs), (173, 238)

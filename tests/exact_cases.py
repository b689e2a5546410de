"""Deterministic cases for the exact-integer path (fr_exact.hip), with the answers of tests/exact_ref.py.

Five tiers, each built once per process by tier(name) -> (jobs, {label: exact_ref.Stats}):

  small     closed contours of 1 to 4 curves in about +-12, 1 to 3 contours per glyph: one-curve contours, horizontal
            runs, shared heights, second differences of exactly 1 (straight at K = 1 only); the whole lattice box +-2 at
            K = 1 and K = 2, windows on curve points at every K from 3 to 8
  limit     the same shapes stretched to multiples of 16 reaching +-32752, some with their extremes at +-32767, and a few
            drawn for wide operands; K = 1 query lists with the +-32767 corners, K = 8 windows centred on exact curve
            points B(j/4), at the four +-2^20 corners and on the +-2^20 edges beside the glyph
  many      255, 256, 257 and 513 curves from many small overlapping contours; one window and query lists of 1, 255,
            256 and 257 points (prefixes of one list)
  coverage  right triangles with a diagonal edge, n = 1 .. 8 lattice points per pixel axis
  colour    two stacks of five nested squares, one per direction (windings -5 .. 5), at scales 1, 63, 64, 85, 86, 255

A job is (kind, glyph, args, expect): "info" (), "query" (points,), "wlattice" (), "lattice" (K, x0, y0, w, h),
"coverage" (K, x0, y0, w_px, h_px, n) and "debug" (scale,).  Glyphs are exact_ref glyphs (lists of contours of integer
points); to_fr() makes the library's Glyph of one.

Measured (one CPU core, CPython 3.10): the whole reference pass, all five tiers (807 jobs) with both counters on, takes
5.0 s (small 2.5, limit 0.9, many 1.3, coverage 0.3); tests/test_exact_ref.py as a whole 9.4 s, 3.6 s of it the crossing
count.  The widest operands compared: small tier dy abxy^2 48 bits and tmp^2 49; limit tier at K = 1 100 and 102 bits, at
K = 8 118 and 123 bits; many 36 and 40.  tests/test_exact_ref.py asserts the bounds these have to reach."""
import functools
import random
import time
from fractions import Fraction

import numpy as np

import exact_ref as R

TIERS = ("small", "limit", "many", "coverage", "colour")
LIM = 1 << 20
COLOUR_SCALES = (1, 63, 64, 85, 86, 255)


class Job:
    def __init__(self, kind, glyph, args, expect, extra=None):
        self.kind, self.glyph, self.args, self.expect, self.extra = kind, glyph, args, expect, extra

    def __repr__(self):
        a = tuple(x if not hasattr(x, "__len__") else "<%d>" % len(x) for x in self.args)
        return "Job(%s, %d curves, %r)" % (self.kind, sum(len(c) // 2 for c in self.glyph), a)


def to_fr(glyph):
    from font_renderer_amd.glyph import Box, Contour, Glyph
    return Glyph(Box(*R.box_of(glyph)), [Contour(np.array(c, np.int16)) for c in glyph])


# ---- shapes ----------------------------------------------------------------------------------------------------------
def _control(rng, a, b, rad):
    """a control point between on-curve points a and b, by one of the ways curves go wrong"""
    mode = rng.choice(("any", "any", "mid", "d2", "d2", "flat", "level", "over0", "over2", "liny"))
    mx, my = (a[0] + b[0]) // 2, (a[1] + b[1]) // 2            # with an odd sum: second difference +1
    if mode == "mid":
        return (mx, my)
    if mode == "d2":                                           # second differences in {-1, 0, 1}, +-1 where the sum is odd
        return (mx + ((a[0] + b[0]) & 1) * rng.randint(0, 1), my + ((a[1] + b[1]) & 1) * rng.randint(0, 1))
    x = rng.randint(-rad, rad)
    if mode == "flat":
        return (x, a[1])
    if mode == "level":
        return (x, b[1])
    if mode == "over0":                                        # beyond p0's height, away from p2
        d = rng.randint(1, 4) * (1 if a[1] >= b[1] else -1)
        return (x, max(-rad, min(rad, a[1] + d)))
    if mode == "over2":
        d = rng.randint(1, 4) * (1 if b[1] >= a[1] else -1)
        return (x, max(-rad, min(rad, b[1] + d)))
    if mode == "liny" and (a[1] + b[1]) % 2 == 0:              # linear in y, bent in x
        return (x, my)
    return (x, rng.randint(-rad, rad))


def _contour(rng, n, rad, heights, off=(0, 0)):
    on = []
    for _ in range(n):
        y = rng.choice(heights) if rng.random() < 0.5 else rng.randint(-rad, rad)
        on.append((rng.randint(-rad, rad), y))
    pts = []
    for k in range(n):
        a, b = on[k], on[(k + 1) % n]
        pts += [a, _control(rng, a, b, rad)]
    pts.append(on[0])
    return [(x + off[0], y + off[1]) for (x, y) in pts]


def _small_glyph(rng, rad=12):
    heights = [rng.randint(-rad, rad) for _ in range(3)]
    sizes = [rng.choice((1, 2, 3, 3, 4, 4)) for _ in range(rng.randint(1, 3))]
    return [_contour(rng, n, rad, heights) for n in sizes]


N_SMALL = 72


@functools.lru_cache(None)
def small_glyphs():
    rng = random.Random(0x5EED0001)
    gl = [_small_glyph(rng) for _ in range(N_SMALL)]
    # a lone one-curve contour, and a horizontal run before a curve that leaves its start point upwards and downwards
    gl.append([[(-3, 2), (4, -6), (-3, 2)]])
    gl.append([[(-6, 0), (-2, 0), (2, 0), (5, 4), (6, 8), (0, 9), (-6, 8), (-6, 4), (-6, 0)],
               [(8, 3), (5, 3), (2, 3), (2, -1), (3, -5), (9, -2), (8, 3)]])
    return gl


def _stretch(glyph, top):
    def f(c):
        return (top if c > 0 else -top) if abs(c) == 12 else 2720 * c
    return [[(f(x), f(y)) for (x, y) in c] for c in glyph]


@functools.lru_cache(None)
def limit_glyphs():
    m, e = 32767, 32752
    gl = [_stretch(g, 32767 if i % 4 == 3 else 32752) for i, g in enumerate(small_glyphs()[:28])]
    # drawn for wide operands: control points a whole box away from their chords
    gl.append([[(-m, m), (m, -m), (m, m), (0, m), (-m, m)]])
    gl.append([[(e, -e), (-e, e), (e, -e + 16), (e, -e + 8), (e, -e)]])
    gl.append([[(-e, -e), (e, e), (-e, e), (-e, 0), (-e, -e)], [(m, m), (-m, -m), (m, -m), (m, 1), (m, m)]])
    gl.append([[(-m, -m), (-m, m), (m, m), (m, -m), (-m, -m)]])
    gl.append([[(-e, e), (e, -e), (-e, e - 32), (-e, e - 16), (-e, e)], [(e, 0), (-e, e), (-e, 16), (0, 0), (e, 0)]])
    return gl


MANY_SIZES = {255: [3] * 85, 256: [4] + [3] * 84, 257: [2] + [3] * 85, 513: [3] * 171}     # curve 256 is a triangle's side


@functools.lru_cache(None)
def many_glyphs():
    out = {}
    for n, sizes in MANY_SIZES.items():
        rng = random.Random(0x5EED0100 + n)
        g = []
        for s in sizes:
            off = (rng.randint(-8, 8), rng.randint(-8, 8))
            g.append(_contour(rng, s, 3, [0, 1], off))
        assert sum(len(c) // 2 for c in g) == n
        out[n] = g
    return out


def _triangle(a, b):
    return [[(0, 0), (a // 2, 0), (a, 0), (a // 2, b // 2), (0, b), (0, b // 2), (0, 0)]]


TRIANGLES = ((58, 46), (36, 60), (62, 22), (44, 58))


def colour_glyph():
    g = []
    for cx, turn in ((-8, 1), (8, -1)):
        for h in (6, 5, 4, 3, 2):
            c = [(cx - h, -h), (cx, -h), (cx + h, -h), (cx + h, 0), (cx + h, h), (cx, h), (cx - h, h), (cx - h, 0), (cx - h, -h)]
            g.append(c if turn > 0 else c[::-1])
    return g


def curve_points(glyph, K):
    """the points B(j/4), j = 1, 2, 3, of every curve of the K-times scaled glyph that are lattice points"""
    out = []
    for (_, _, p0, p1, p2) in R.curves_of(glyph, K):
        for j in (1, 2, 3):
            x = Fraction((4 - j) ** 2 * p0[0] + 2 * j * (4 - j) * p1[0] + j * j * p2[0], 16)
            y = Fraction((4 - j) ** 2 * p0[1] + 2 * j * (4 - j) * p1[1] + j * j * p2[1], 16)
            if x.denominator == 1 and y.denominator == 1:
                out.append((int(x), int(y)))
    return out


# ---- jobs ------------------------------------------------------------------------------------------------------------
def _lattice(glyph, K, x0, y0, w, h, st):
    assert 1 <= w <= 64 and 1 <= h <= 64 and -LIM <= x0 and x0 + w <= LIM and y0 <= LIM and y0 - h >= -LIM
    return Job("lattice", glyph, (K, x0, y0, w, h), np.array(R.exact_lattice(glyph, K, x0, y0, w, h, st), np.int16))


def _centred(glyph, K, c, w, h, st):
    x0 = max(-LIM, min(LIM - w, c[0] - w // 2))
    y0 = min(LIM, max(-LIM + h, c[1] + h // 2))
    return _lattice(glyph, K, x0, y0, w, h, st)


def _info(glyph):
    ct, ip = R.glyph_info(glyph, 1)
    return Job("info", glyph, (), (np.array(ct, np.uint8), np.array(ip, np.uint8)))


def _small():
    st = {"small": R.Stats()}
    s, jobs = st["small"], []
    for i, g in enumerate(small_glyphs()):
        b = R.box_of(g)
        jobs.append(_info(g))
        for K in (1, 2):
            jobs.append(_lattice(g, K, K * (b[0] - 2), K * (b[3] + 2), K * (b[2] - b[0] + 4) + 1, K * (b[3] - b[1] + 4) + 1, s))
        if i % 4 == 0:
            jobs.append(Job("wlattice", g, (), np.array(R.winding_lattice(g, b, s), np.int16)))
        K = (3, 8, 4, 5, 8, 6, 7, 8)[i % 8]
        on = curve_points(g, K) or [(K * g[0][0][0], K * g[0][0][1])]
        jobs.append(_centred(g, K, on[i % len(on)], 33, 31, s))
    return jobs, st


def _limit():
    st = {"limit_k1": R.Stats(), "limit_k8": R.Stats()}
    s1, s8, jobs = st["limit_k1"], st["limit_k8"], []
    rng = random.Random(0x5EED0200)
    m = 32767
    for i, g in enumerate(limit_glyphs()):
        jobs.append(_info(g))
        on1 = curve_points(g, 1)
        vs = [c[2 * k] for c in g for k in range(len(c) // 2)]
        q = [(sx * m, sy * m) for sx in (-1, 1) for sy in (-1, 1)]
        for (x, y) in on1 + vs:
            q += [(x, y), (min(m, x + 1), y), (max(-m, x - 1), y), (x, min(m, y + 1)), (x, max(-m, y - 1)), (-m, y), (m, y)]
        q += [(rng.randint(-m, m), rng.randint(-m, m)) for _ in range(40)]
        jobs.append(Job("query", g, (q,), np.array(R.winding_in_glyph(g, q, s1), np.int16)))
        on8 = curve_points(g, 8)
        for c in on8[i % 3::max(1, len(on8) // 8)][:8]:       # a spread of the curve points, not all of them
            jobs.append(_centred(g, 8, c, 9, 9, s8))
        c = on8[i % len(on8)]
        if i % 3 == 0:
            jobs.append(_centred(g, 8, c, 64, 64, s8))
        for x in (-LIM, LIM):                                 # the far edges, on the height of a curve point
            jobs.append(_centred(g, 8, (x, c[1]), 8, 8, s8))
        if i % 4 == 1:
            for x in (-LIM, LIM):
                for y in (-LIM, LIM):
                    jobs.append(_centred(g, 8, (x, y), 8, 8, s8))
    return jobs, st


def _many():
    st = {"many": R.Stats()}
    s, jobs = st["many"], []
    for n, g in many_glyphs().items():
        rng = random.Random(0x5EED0300 + n)
        jobs.append(_info(g))
        jobs.append(_lattice(g, 1, -12, 12, 25, 23, s))
        q = [(rng.randint(-12, 12), rng.randint(-12, 12)) for _ in range(257)]
        full = np.array(R.winding_in_glyph(g, q, s), np.int16)
        for k in (1, 255, 256, 257):
            jobs.append(Job("query", g, (q[:k],), full[:k].copy()))
    jobs.append(_lattice(many_glyphs()[257], 8, -40, 36, 37, 29, s))
    return jobs, st


def _coverage():
    st = {"coverage": R.Stats()}
    jobs = []
    for n in range(1, 9):
        for (a, b) in TRIANGLES:
            g, px = _triangle(a, b), 64 // n
            args = (1, -2, b + 2, px, px, n)
            cov, counts = R.exact_coverage(g, *args, stats=st["coverage"])
            jobs.append(Job("coverage", g, args, np.array(cov, np.uint8), extra=counts))
    g = _triangle(12, 10)                                      # the refined lattice: 1/8 unit between points
    args = (8, -16, 88, 16, 13, 4)
    jobs.append(Job("coverage", g, args, np.array(R.exact_coverage(g, *args, stats=st["coverage"])[0], np.uint8)))
    return jobs, st


def _colour():
    st = {"colour": R.Stats()}
    g = colour_glyph()
    b = R.box_of(g)
    lat = R.winding_lattice(g, b, st["colour"])
    jobs = [_info(g), Job("wlattice", g, (), np.array(lat, np.int16))]
    for scale in COLOUR_SCALES:
        jobs.append(Job("debug", g, (scale,), np.array(R.debug_render(g, b, scale, lat), np.uint8)))
    return jobs, st


SECONDS = {}


@functools.lru_cache(None)
def tier(name):
    t = time.perf_counter()
    out = {"small": _small, "limit": _limit, "many": _many, "coverage": _coverage, "colour": _colour}[name]()
    SECONDS[name] = time.perf_counter() - t
    return out


def all_stats():
    total = R.Stats()
    for name in TIERS:
        for s in tier(name)[1].values():
            total.merge(s)
    return total

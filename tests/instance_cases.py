"""The raster kernels' instance matrix: one tiny plan per kernel instance the dispatcher can launch, and a predictor
of the instance a plan gets.  Pure Python: no GPU, no library call.

The raster side is one algorithm compiled into 246 instances (fr_cov4.hip, fr_win1.hip, fr_render.hip); which one a
job gets is decided on the host in fr_raster_plan.cpp (fast_rule, fast_class, merge_small_classes and, for the
instance's template arguments, raster_launches), which also names it (raster_launch_name).  `predicted_name` restates
those rules, glyph_root_bound and glyph_ray_bound included, and returns the
string fr_plan_describe prints for the plan's kernel.  `expected_instances` is written from the template parameter
products alone, independently of the case table; tests/test_instance_cases.py holds the two together and
tests/test_gpu_instances.py renders every case against a CPU reference."""
import functools
from collections import namedtuple

import numpy as np

from font_renderer_amd.glyph import Box, Contour, Glyph, GlyphSet
from font_renderer_amd.synth import _div_trunc2, comb_glyph, stroke_glyphset, synth_glyphset

# fr_mode (include/fr_raster.h)
WINDING_I16, GRAY_DEBUG, MASK_NONZERO, COVERAGE_U8, SDF_U8 = 0, 1, 2, 3, 4
# render_kernel's MODE (fr_render.hip) and win1_kernel's (fr_win1.hip)
R_WINDING, R_GRAY, R_COVERAGE = 0, 1, 3
W1_MODES = (0, 1, 2, 3)                      # winding_i16, gray_debug, mask, sign bits (FR_SDF_U8)

JOB_DTYPE = np.dtype([("glyph", "<u4"), ("min_x", "<i4"), ("max_y", "<i4"), ("w", "<u4"), ("h", "<u4"),
                      ("out_x", "<u4"), ("out_y", "<u4"), ("scale", "<f4")])

# A case: family "cov4" / "win1" / "render" (render: option cov4 = 0), the fr_raster_params (mode, n, center), the
# _ex flag (fill), option kmax, the glyphs (a GlyphSet) and the job table (JOB_DTYPE) with the output array's shape.
# key: the template parameters the case was built for — the predictor never reads it.
Case = namedtuple("Case", "family mode n fill kmax center gs jobs shape key")


# ---- the host rules (fr_raster_plan.cpp) --------------------------------------------------------------------------
def glyph_segments(gs, g):
    """(S, 3, 2) int64: p0, p1, p2 of every segment of glyph g"""
    out = []
    for c in range(int(gs.glyph_start[g]), int(gs.glyph_start[g + 1])):
        p = gs.points_xy[int(gs.contour_start[c]):int(gs.contour_start[c + 1])].astype(np.int64)
        for k in range(len(p) // 2):
            out.append(p[2 * k:2 * k + 3])
    return np.array(out, np.int64).reshape(-1, 3, 2)


def root_bound(segs):
    """glyph_root_bound: the two candidate roots of a segment minus those the vertex rule discards unseen"""
    nb = 0
    for (_, p0y), (_, p1y), (_, p2y) in segs.tolist():
        a, b = p0y - 2 * p1y + p2y, p0y - p1y
        if a == 0:
            nb += 1 if p2y != p0y else 0
            continue
        tv_lt0 = b * a < 0
        tv_ge1 = (b >= a) if a > 0 else (b <= a)
        nb += (0 if tv_ge1 else 1) + (0 if tv_lt0 else 1)
    return nb


def ray_bound(segs):
    """glyph_ray_bound: a sweep over the segments' y extents, once between the ends' heights, twice where the control
    point overshoots them (by half of its own overshoot); events sort as (2 y + [closing], weight) pairs"""
    ev = []
    for (_, p0y), (_, p1y), (_, p2y) in segs.tolist():
        clo, chi = min(p0y, p2y), max(p0y, p2y)
        ev.append((2 * clo, 1))
        ev.append((2 * chi, -1))
        if p1y > chi:
            ev.append((2 * chi, 2))
            ev.append((2 * (chi + (p1y - chi + 1) // 2) + 1, -2))
        if p1y < clo:
            ev.append((2 * (clo - (clo - p1y + 1) // 2), 2))
            ev.append((2 * clo, -2))
    cur = best = 0
    for _, wgt in sorted(ev):
        cur += wgt
        best = max(best, cur)
    return best


def fast_ns(family, mode, n):
    """fast_rule with the default strip_px: samples per axis on the fast kernels, 0 = the plan has none"""
    if family == "render":                   # option cov4 = 0
        return 0
    if mode in (WINDING_I16, GRAY_DEBUG, MASK_NONZERO, SDF_U8) or (mode == COVERAGE_U8 and n == 1):
        return 1
    return n if (mode == COVERAGE_U8 and n in (2, 4)) else 0


def fast_class(ns, w, h, nsg, rootb, rayb):
    """fast_class: 0 (the general kernel) or 1 + 4 (wlog - 2) + record class"""
    if not ns or w == 0 or h == 0 or h * ns > 2048:
        return 0
    if nsg > 768 or rootb > 1024:
        return 0
    wl = 2 if w <= 64 else (3 if w <= 128 else 4)
    if nsg <= 256 and rootb <= 128 and rayb <= 16:
        rc = 0
    elif nsg <= 256 and rootb <= 256:
        rc = 1
    elif nsg <= 384 and rootb <= 512:
        rc = 2
    else:
        rc = 3
    return 1 + 4 * (wl - 2) + rc


def job_classes(case):
    ns = fast_ns(case.family, case.mode, case.n)
    out = []
    for j in case.jobs:
        segs = glyph_segments(case.gs, int(j["glyph"]))
        out.append(fast_class(ns, int(j["w"]), int(j["h"]), len(segs), root_bound(segs), ray_bound(segs)))
    return out


def _cap(kmax):
    return 8 if kmax <= 8 else (16 if kmax <= 16 else 32)


def predicted_name(case):
    """the first kernel name fr_plan_describe prints for the case's plan.  The plan must be single-class (a plan's only
    class is left alone by merge_small_classes); raises otherwise."""
    classes = set(job_classes(case))
    if len(classes) != 1:
        raise ValueError(f"jobs of classes {sorted(classes)} in one case")
    cls = classes.pop()
    tail = ", 1>" if case.fill else ">"
    if cls:
        wlog, rpl = 2 + (cls - 1) // 4, 2 << ((cls - 1) % 4)
        if fast_ns(case.family, case.mode, case.n) == 1:                       # raster_launches: a fast part
            m = {WINDING_I16: 0, GRAY_DEBUG: 1, SDF_U8: 3}.get(case.mode, 2)
            return f"fr::win1_kernel<{wlog}, {m}, {rpl}{tail}"
        kmax = 16 if (rpl == 2 and case.kmax > 16) else case.kmax              # (its two exceptions for CAP)
        cap = 32 if rpl >= 16 else _cap(kmax)
        return f"fr::cov4_kernel<{wlog}, {cap}, {rpl}, {case.n}{tail}"
    # the general kernel: strip width from the widest job, uniform = every strip and every wave band full
    gmax_w = max(int(j["w"]) for j in case.jobs)
    sw = min((gmax_w + 15) & ~15, 256) or 16
    band = 64 // case.n
    uniform = all(int(j["w"]) and int(j["h"]) and int(j["w"]) % sw == 0 and int(j["h"]) % band == 0 for j in case.jobs)
    if case.mode == COVERAGE_U8:
        mode, n = R_COVERAGE, case.n
    elif case.mode in (MASK_NONZERO, SDF_U8):                                  # 1-sample coverage is the mask
        mode, n = R_COVERAGE, 1
    else:
        mode, n = (R_WINDING if case.mode == WINDING_I16 else R_GRAY), 1
    wlog = -1
    if mode == R_COVERAGE and n == 4 and uniform and sw in (256, 128):
        wlog = 4 if sw == 256 else 3
    return f"fr::render_kernel<{mode}, {n}, {_cap(case.kmax)}, {wlog}{tail}"


# ---- the expected instance set: the template parameter products, nothing from the case table ------------------------
COV4_RPL_CAP = ((2, 8), (2, 16), (4, 8), (4, 16), (4, 32), (8, 8), (8, 16), (8, 32), (16, 32))
RENDER_MNW = ((R_COVERAGE, 1, -1), (R_COVERAGE, 2, -1), (R_COVERAGE, 4, -1), (R_COVERAGE, 4, 4), (R_COVERAGE, 4, 3),
              (R_WINDING, 1, -1), (R_GRAY, 1, -1))


def expected_instances():
    names = []
    for tail in (">", ", 1>"):
        for wlog in (2, 3, 4):
            for rpl, cap in COV4_RPL_CAP:
                for ns in (2, 4):
                    names.append(f"fr::cov4_kernel<{wlog}, {cap}, {rpl}, {ns}{tail}")
            for mode in W1_MODES:
                for rpl in (2, 4, 8, 16):
                    names.append(f"fr::win1_kernel<{wlog}, {mode}, {rpl}{tail}")
        for mode, n, wlog in RENDER_MNW:
            for cap in (8, 16, 32):
                names.append(f"fr::render_kernel<{mode}, {n}, {cap}, {wlog}{tail}")
    return names


# instances no plan of the public API can reach: (name, the line of the C ABI units, csrc/fr_api_*.hip, that proves it).  None found.
UNREACHABLE = []


# ---- glyphs ---------------------------------------------------------------------------------------------------------
def comb_contour(teeth, x0, y0, width, height, valley):
    """synth.comb_glyph's polygon with every measure free: `teeth` teeth over [y0 + valley, y0 + height) on a base
    from y0, straight edges with truncated midpoints"""
    pitch = width // teeth
    poly = [(x0, y0)]
    for t in range(teeth):
        xa = x0 + t * pitch
        xb = xa + pitch // 2
        poly += [(xa, y0 + height), (xb, y0 + height), (xb, y0 + valley), (xa + pitch, y0 + valley)]
    poly += [(x0 + teeth * pitch, y0)]
    poly = np.array(poly, np.int64)
    pts = np.empty((2 * len(poly) + 1, 2), np.int64)
    pts[0:-1:2] = poly
    pts[1:-1:2] = _div_trunc2(poly + np.roll(poly, -1, 0))
    pts[-1] = poly[0]
    return pts.astype(np.int16)


COMB_ROWS = (300, 1600)          # comb_glyph(T): a ray at 300 <= y < 1600 meets its 2 T vertical edges
BALLAST_Y = (1750, 1950)         # the ballast contour: above the comb (100 .. 1600), teeth over y in [1850, 1950)
BALLAST_TEETH = (0, 10, 70, 120)    # per record class: what lifts comb_glyph(T), T <= 17, into it (the predictor decides)


def comb_ballast_glyph(teeth, ballast):
    """comb_glyph(teeth) plus, when ballast > 0, a second contour above its rows: a low comb of `ballast` teeth that
    only raises the segment, root-record and ray counts to the wanted record class"""
    cs, _ = comb_glyph(teeth)
    cs = [np.asarray(c, np.int16) for c in cs]
    if ballast:
        cs.append(comb_contour(ballast, 100, BALLAST_Y[0], 1800, BALLAST_Y[1] - BALLAST_Y[0], 100))
    allp = np.concatenate(cs)
    box = Box(int(allp[:, 0].min()), int(allp[:, 1].min()), int(allp[:, 0].max()), int(allp[:, 1].max()))
    return Glyph(box, [Contour(c) for c in cs])


# the curved glyph of a record class: (maker, segments); 256-segment-and-under sets land in classes 0 / 1 by their
# root and ray bounds, 300 segments need the 512-record class, 500 the 1024-record one
CURVED = ((synth_glyphset, 56), (synth_glyphset, 128), (synth_glyphset, 300), (synth_glyphset, 500))
CURVED_ALT3 = (stroke_glyphset, 768)      # every other class-3 case: stroke-dense, the segment limit itself


@functools.lru_cache(maxsize=None)
def _curved_glyph(rc, index):
    """the first glyph of the class's generator, from a seed fixed by the case index on, that the host rules put into
    record class rc (the segment counts above are where to look; the predictor decides)"""
    make, segs = CURVED_ALT3 if (rc == 3 and index % 2) else CURVED[rc]
    for k in range(64):
        gs = make(1, segs, first_index=1000 + 7 * index + 1009 * k)
        s = glyph_segments(gs, 0)
        if fast_class(4, 64, 16, len(s), root_bound(s), ray_bound(s)) == 1 + rc:
            return gs.glyph(0)
    raise ValueError(f"no {make.__name__}({segs}) glyph of record class {rc}")


# ---- cells ----------------------------------------------------------------------------------------------------------
WIDTHS = {2: 61, 3: 125, 4: 261}          # WLOG -> cell width: ragged strips; 261 makes a second strip of 5 pixels
COMB_SCALE = {2: 1.0 / 32, 3: 1.0 / 16, 4: 1.0 / 8}     # the comb (x <= 1900) ends inside the first strip; dyadic:
#                                                         sample rows fall exactly on the combs' vertex heights
SENTINEL = 0x5b
OUT_X0, OUT_Y0, GAP = 3, 2, 5             # odd out_x, a sentinel border on every side, odd gaps between the cells


def cell_height(n):
    """five wave bands, the last one ragged: bands of 16 pixel rows for n = 4 and for one sample, 32 for n = 2"""
    return 133 if n == 2 else 69


def _comb_job(g, wlog, w, h):
    s = np.float32(COMB_SCALE[wlog])
    top = int(np.ceil(BALLAST_Y[1] * float(s))) + 2                      # two empty rows, then ballast, then the teeth
    return (g, -1, top, w, h, s)


def _curved_job(g, glyph, w, h):
    """the glyph's top-left part at a scale that pushes its right side out of the cell (clipped strips), three empty
    columns on the left, two empty rows on top"""
    b = glyph.box
    s = np.float32(1.05 * w / max(1, b.x_max - b.x_min))
    return (g, int(np.floor(b.x_min * float(s))) - 3, int(np.ceil(b.y_max * float(s))) + 2, w, h, s)


def _place(rows):
    """(glyph, min_x, max_y, w, h, scale) rows side by side -> (job table, output shape): odd out_x, a stride that is
    no multiple of 16, sentinels on every side"""
    jobs = np.zeros(len(rows), JOB_DTYPE)
    x = OUT_X0
    for i, (g, min_x, max_y, w, h, s) in enumerate(rows):
        jobs[i] = (g, min_x, max_y, w, h, x, OUT_Y0, s)
        x += w + GAP + (w + GAP) % 2                                     # keeps out_x odd
    stride = x + 2
    stride += 1 if stride % 16 == 0 else 0
    return jobs, (OUT_Y0 + max(r[4] for r in rows) + 3, stride)


def _comb_teeth(family, rpl, cap):
    """the combs of a case: a sample row that meets exactly CAP crossings and one that meets CAP + 2 — but the
    two-records-per-lane class holds glyphs of <= 16 crossings per ray only, and win1_kernel has no CAP: 16 and 34
    crossings, either side of the 31 a row of byte differences holds"""
    if family == "win1":
        return (8,) if rpl == 2 else (8, 17)
    if rpl == 2 and cap == 16:
        return (8,)
    return (cap // 2, cap // 2 + 1)


def _make_case(index, family, mode, n, fill, kmax, center, wlog, rc, cap, key, uniform_cell=None):
    if uniform_cell:
        w, h = uniform_cell
    else:
        w, h = WIDTHS[wlog], cell_height(n)
    rpl = 2 << rc
    glyphs = [_curved_glyph(rc, index)]
    rows = [_curved_job(0, glyphs[0], w, h)]
    for t in _comb_teeth(family, rpl if family != "render" else 0, cap):
        glyphs.append(comb_ballast_glyph(t, BALLAST_TEETH[rc]))
        rows.append(_comb_job(len(glyphs) - 1, wlog, w, h))
    jobs, shape = _place(rows)
    return Case(family, mode, n, fill, kmax, center, GlyphSet(glyphs), jobs, shape, key)


@functools.lru_cache(maxsize=None)
def build_cases():
    """one case per instance.  The sample phase alternates with the case index inside every (family, NS or MODE, FILL)
    group — each group has several cases, so both phases occur in it."""
    cases = []
    for fill in (0, 1):
        for ns in (2, 4):
            i = 0
            for wlog in (2, 3, 4):
                for rpl, cap in COV4_RPL_CAP:
                    rc = {2: 0, 4: 1, 8: 2, 16: 3}[rpl]
                    cases.append(_make_case(i, "cov4", COVERAGE_U8, ns, fill, cap, i % 2 == 1, wlog, rc, cap,
                                            ("cov4", wlog, cap, rpl, ns, fill)))
                    i += 1
        for m in W1_MODES:
            mode = (WINDING_I16, GRAY_DEBUG, MASK_NONZERO, SDF_U8)[m]
            i = 0
            for wlog in (2, 3, 4):
                for rc in range(4):
                    cases.append(_make_case(i, "win1", mode, 1, fill, 32, (i + wlog) % 2 == 1, wlog, rc, 0,
                                            ("win1", wlog, m, 2 << rc, fill)))
                    i += 1
        for rmode, n, rw in RENDER_MNW:
            mode = {R_COVERAGE: COVERAGE_U8, R_WINDING: WINDING_I16, R_GRAY: GRAY_DEBUG}[rmode]
            for i, cap in enumerate((8, 16, 32)):
                # ragged cells of another width and record class per CAP; the two uniform instances need uniform plans
                cell = {4: (256, 64), 3: (128, 64)}.get(rw)
                wlog = rw if rw > 0 else 2 + (i + n) % 3
                cases.append(_make_case(i + n, "render", mode, n, fill, cap, (i + (rw > 0)) % 2 == 1, wlog, (i + n) % 4, cap,
                                        ("render", rmode, n, cap, rw, fill), uniform_cell=cell))
    return tuple(cases)


def group_of(case):
    """(family, NS or MODE, FILL): what tests/test_gpu_instances.py is parametrised by"""
    k = case.key
    if case.family == "cov4":
        return ("cov4", k[4], k[5])
    if case.family == "win1":
        return ("win1", k[2], k[4])
    return ("render", f"{k[1]}.{k[2]}", k[5])


def groups():
    out = []
    for fill in (0, 1):
        out += [("cov4", ns, fill) for ns in (2, 4)]
        out += [("win1", m, fill) for m in W1_MODES]
        out += [("render", f"{m}.{n}", fill) for m, n in sorted({(m, n) for m, n, _ in RENDER_MNW})]
    return out

"""An independent restatement of FR_FILL_CONSISTENT (include/fr_raster.h) in numpy, written
from the rule, not from the kernels:

  1. pieces: a segment with a == 0 is one piece p0 -> p2 (none if p0y == p2y); a quadratic one is split at its
     y-extremum t_v = b / a (b = p0y - p1y) into the y-monotone halves that lie in t in [0, 1]; a piece whose
     y-extent is a single value contributes nothing;
  2. a piece with exact end heights ylo < yhi is crossed at ray height cy iff ylo <= cy < yhi — exact, here with
     fractions.Fraction on cy as the binary32 it is;
  3. the crossing adds -1 if the piece rises along t, +1 if it falls;
  4. xx is the reference's float32 expression (t as render_glyph.zig:51 / :60-61, xx as :53 / :65, one rounding per
     operation, like tests/ref_numpy.py) with delta clamped at 0 before the square root; it counts iff !(xx < cx).

Sample points are the library's (fr_job in include/fr_raster.h), binary32 throughout."""
from fractions import Fraction

import numpy as np

F = np.float32
WINDING_I16, GRAY_DEBUG, MASK_NONZERO, COVERAGE_U8 = 0, 1, 2, 3


def pieces(points_xy, contour_start):
    """every piece of a glyph: (p0, p1, p2 as ints, root, ylo, yhi, sign) with root None for a line, +1 / -1 for
    the t+ / t- half of a quadratic; ylo / yhi exact (int or Fraction); sign = -1 rising, +1 falling"""
    out = []
    for c in range(len(contour_start) - 1):
        p = np.asarray(points_xy[int(contour_start[c]):int(contour_start[c + 1])], np.int64)
        for k in range(len(p) // 2):
            (p0x, p0y), (p1x, p1y), (p2x, p2y) = (tuple(int(v) for v in p[2 * k + i]) for i in range(3))
            seg = ((p0x, p0y), (p1x, p1y), (p2x, p2y))
            a = p0y - 2 * p1y + p2y
            if a == 0:
                if p0y != p2y:
                    out.append((seg, None, min(p0y, p2y), max(p0y, p2y), -1 if p0y < p2y else 1))
                continue
            b = p0y - p1y
            tv = Fraction(b, a)
            yv = p0y - Fraction(b * b, a)

            def y_at(t):
                return p0y - 2 * b * t + a * t * t
            for root in (1, -1):
                # y'(t) = 2 a (t - t_v): the t+ root (a (t - t_v) = +sqrt(delta) >= 0) is the rising half
                after = (root == 1) == (a > 0)            # this half is t >= t_v
                lo_t, hi_t = (max(Fraction(0), tv), Fraction(1)) if after else (Fraction(0), min(Fraction(1), tv))
                if lo_t >= hi_t:
                    continue
                y0, y1 = (yv if lo_t == tv else y_at(lo_t)), (yv if hi_t == tv else y_at(hi_t))
                if y0 == y1:
                    continue
                out.append((seg, root, min(y0, y1), max(y0, y1), -1 if root == 1 else 1))
    return out


def piece_end_heights(points_xy, contour_start):
    """(heights, margins): float64 approximations of every piece's end heights, and for each the distance within which
    the REFERENCE's own float acceptance (render_glyph.zig:58-64) is blurred: 2^-8 font units, or four rounding plateaus
    of delta = cy a + c1 - c2 of the segment, ulp(max(|c1|, |c2|)) / |a|, where that is wider (a nearly straight
    quadratic: |a| of 1 with c1 ~ 2^21 blurs its ends by ~0.5 font units)"""
    out = {}
    for (seg, root, ylo, yhi, _) in pieces(points_xy, contour_start):
        m = 2.0 ** -8
        if root is not None:
            (_, p0y), (_, p1y), (_, p2y) = seg
            a = p0y - 2 * p1y + p2y
            big = float(max(abs(np.float32(p1y * p1y)), abs(np.float32(p0y * p2y)), 1.0))
            m = max(m, 4.0 * float(np.spacing(np.float32(big))) / abs(a))
        for v in (float(ylo), float(yhi)):
            out[v] = max(out.get(v, 0.0), m)
    hs = sorted(out)
    return np.array(hs, np.float64), np.array([out[h] for h in hs], np.float64)


def _crossed_rows(cy_unique, ylo, yhi):
    """ylo <= cy < yhi, exact, for each distinct binary32 ray height"""
    lo_f, hi_f = float(ylo), float(yhi)
    res = np.zeros(len(cy_unique), bool)
    sure = (cy_unique > lo_f + 1.0) & (cy_unique < hi_f - 1.0)     # (ends are >= 1 apart or exactly compared below)
    res[sure] = True
    near = ~sure & (cy_unique >= lo_f - 1.0) & (cy_unique <= hi_f + 1.0)
    for i in np.nonzero(near)[0]:
        c = Fraction(float(cy_unique[i]))
        res[i] = ylo <= c < yhi
    return res


def winding_fill(points_xy, contour_start, cx, cy):
    """winding numbers under FR_FILL_CONSISTENT at the binary32 sample points (cx, cy) (broadcastable arrays)"""
    cx = np.asarray(cx, F)
    cy = np.asarray(cy, F)
    shape = np.broadcast(cx, cy).shape
    w = np.zeros(shape, np.int32)
    cyu, inv = np.unique(cy, return_inverse=True)
    inv = inv.reshape(cy.shape)
    two, zero = F(2), F(0)
    with np.errstate(all="ignore"):
        for (seg, root, ylo, yhi, sgn) in pieces(points_xy, contour_start):
            acc_u = _crossed_rows(cyu, ylo, yhi)
            if not acc_u.any():
                continue
            acc = acc_u[inv]
            (p0x, p0y), (p1x, p1y), (p2x, p2y) = ((F(x), F(y)) for x, y in seg)
            a = F(F(p0y - F(two * p1y)) + p2y)
            ax = F(F(p0x - F(two * p1x)) + p2x)
            bx = F(two * F(p1x - p0x))
            if root is None:
                t = (cy - p0y) / F(p2y - p0y)
            else:
                delta = np.maximum(cy * a + F(p1y * p1y) - F(p0y * p2y), zero)
                sq = np.sqrt(delta).astype(F)
                b = F(p0y - p1y)
                t = ((b + sq) if root == 1 else (b - sq)) / a
            xx = (ax * t + bx) * t + p0x
            w += np.where(acc & ~(xx < cx), sgn, 0).astype(np.int32)
    return w


def sample_axes(min_x, max_y, w, h, scale, n=1, center=False):
    """(cx (w n,), cy (h n,)) of a cell: cx = (f32(min_x + x) + (i + phase)/n) / scale, cy likewise (fr_job)"""
    ph = 0.5 if center else 0.0
    off = np.array([(k + ph) / n for k in range(n)], F)
    s = F(scale)
    xs = (np.arange(w, dtype=np.int64) + min_x).astype(F)
    ys = (max_y - np.arange(h, dtype=np.int64)).astype(F)
    cx = ((xs[:, None] + off[None, :]).reshape(-1)) / s
    cy = ((ys[:, None] - off[None, :]).reshape(-1)) / s
    return cx.astype(F), cy.astype(F)


def to_mode(wd, mode, n=1):
    """sample windings (h n, w n) -> the output of `mode` (fr_mode in include/fr_raster.h)"""
    if mode == WINDING_I16:
        return wd.astype(np.int16)
    if mode == GRAY_DEBUG:
        return np.clip(wd * 20 + 100, 0, 255).astype(np.uint8)
    if mode == MASK_NONZERO:
        return np.where(wd != 0, 255, 0).astype(np.uint8)
    assert mode == COVERAGE_U8
    h, w = wd.shape[0] // n, wd.shape[1] // n
    k = (wd != 0).reshape(h, n, w, n).sum(axis=(1, 3)).astype(np.int64)
    return ((510 * k + n * n) // (2 * n * n)).astype(np.uint8)          # round_half_up(255 k / n^2)


def render_cell(points_xy, contour_start, min_x, max_y, w, h, scale, mode, n=1, center=False):
    cx, cy = sample_axes(min_x, max_y, w, h, scale, n, center)
    return to_mode(winding_fill(points_xy, contour_start, cx[None, :], cy[:, None]), mode, n)


def glyph_dims(box, upm, font_size):
    """render_glyph.zig:13-19 in binary32 -> (min_x, max_y, w, h, scale)"""
    scale = F(font_size) / F(upm)
    b = np.asarray(box, np.int16).astype(F) * scale
    mn0, mn1 = int(np.floor(b[0])), int(np.floor(b[1]))
    mx0, mx1 = int(np.ceil(b[2])), int(np.ceil(b[3]))
    return mn0, mx1, mx0 - mn0 + 1, mx1 - mn1 + 1, scale


def render_glyph(points_xy, contour_start, box, upm, font_size, mode=GRAY_DEBUG):
    """renderGlyph's image (FR_SAMPLE_CORNER, n = 1) under FR_FILL_CONSISTENT"""
    min_x, max_y, w, h, scale = glyph_dims(box, upm, font_size)
    return render_cell(points_xy, contour_start, min_x, max_y, w, h, scale, mode)


def render_batch(gs, jobs, mode, out, n=1, center=False, rows=None):
    """every job of a fr_job table into `out` (as fr_render_batch); rows: optional per-job sample-row subset is not
    supported here — see render_cell for subsampled checks"""
    for j in jobs:
        g = int(j["glyph"])
        c0, c1 = int(gs.glyph_start[g]), int(gs.glyph_start[g + 1])
        p0 = int(gs.contour_start[c0])
        pts = gs.points_xy[p0:int(gs.contour_start[c1])]
        cs = gs.contour_start[c0:c1 + 1] - np.uint32(p0)
        img = render_cell(pts, cs, int(j["min_x"]), int(j["max_y"]), int(j["w"]), int(j["h"]), j["scale"], mode, n, center)
        oy, ox = int(j["out_y"]), int(j["out_x"])
        out[oy:oy + img.shape[0], ox:ox + img.shape[1]] = img
    return out

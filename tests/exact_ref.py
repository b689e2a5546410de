"""The exact-integer winding path (include/fr_raster.h "exact-integer path", DESIGN.md section 6, the comments of
fr_exact.hip) restated in unbounded Python ints, written from the rules and not from the kernels or the C oracle:

  glyph: a list of contours; a contour is a list of 2 n + 1 integer points (x, y), even index on the curve, odd index a
  control point, last == first.  Curve k is (P[2k], P[2k+1], P[2k+2]); every rule is applied to the glyph whose points
  are multiplied by K.

  1. curve type, from the heights of the three points and the second differences d2x = p0x + p2x - 2 p1x, d2y likewise:
     p0y == p2y: x_axis if p1y is on that height too, else balance.  Otherwise the curve goes up (p0y < p2y) or down;
     it is "straight" if |d2x| <= 1 and |d2y| <= 1, "normal" if p1y lies between the end heights (ends included), else a
     U: up_u / down_inv_u overshoot at the p0 end (p1y beyond p0y), up_inv_u / down_u at the p2 end.
  2. include_p0: with (p_2, p_1) the on-curve and control point of the previous curve of the contour (the last curve
     for the first), prev_end = 2 sgn(p0y - p_1y) + sgn(p0y - p_2y), curr_start = 2 sgn(p1y - p0y) + sgn(p2y - p0y):
     include_p0 = curr_start != 0 and (prev_end == 0 or (prev_end > 0) != (curr_start < 0)).
  3. the two predicates share  ay = d2y, by = 2 (p1y - p0y), cy = p0y - py  (so y(t) - py = ay t^2 + by t + cy), the
     same in x, dy = by^2 - 4 ay cy, abxy = ax by - ay bx, tmp = 2 ay (ax cy - ay cx) - by abxy, l = dy abxy^2,
     r = tmp^2.  two_roots: 0 if dy <= 0 or abxy == 0; else s = sgn(abxy) if tmp == 0; else for tmp > 0: 0 if l < r
     else s; for tmp < 0: 0 if l <= r else s.  one_root(tilt_up): False if dy == 0; tmp <= 0 if abxy == 0; if
     (abxy > 0) != tilt_up: True if tmp <= 0 else l >= r; otherwise False if tmp >= 0 else l <= r.
  4. per curve and point p (arms named as the counters name them):
       x_axis                nothing
       balance               row (include_p0 and py == p0y): px < p0x gives +1 if p1y < p0y else -1;
                             else two_roots on the side of p0y the control point is on (p1y >= p0y: py >= p0y)
       up_straight/normal    inside (p0y < py < p2y) or at_p0 (py == p0y, include_p0): -1 if the chord test
                             (py - p0y)(p2x - p0x) >= (px - p0x)(p2y - p0y), resp. one_root(up), holds
       down_straight/normal  the mirror: +1 if (py - p0y)(p2x - p0x) <= (px - p0x)(p2y - p0y), resp. one_root(down)
       up_inv_u              p0y < py <= p2y (inside, at_p2) or at_p0 with include_p0: -1 if one_root(up);
                             py > p2y: two_roots
       down_u                p2y <= py < p0y or at_p0 with include_p0: +1 if one_root(down); py < p2y: two_roots
       up_u                  p0y < py < p2y: -1 if one_root(up); py == p0y: with include_p0 and
                             cross != (px <= p0x): -1 if cross else +1; py < p0y: two_roots
       down_inv_u            p2y < py < p0y: MINUS 1 if one_root(down) (kept as the reference has it); py == p0y: with
                             include_p0 and cross != (px > p0x): +1 if cross else -1; py > p0y: two_roots
  5. the winding of a glyph at p is the sum over its curves; a lattice is the points (x0 + i, y0 - j); coverage is
     round_half_up(255 inside / n^2) over the n x n lattice points of a pixel, inside = winding != 0; the debug colour of
     a winding v at scale s is c = min(|v| s, 65535), main = min(c, 255), sub = 0 if c == main else 150, blue
     (sub, sub, main) for v > 0 and red (main, sub, sub) otherwise; the debug image marks every curve's p0 (255, 255, 0)
     and control point (0, 255, 255) afterwards, in order.

Two optional counters are filled here and nowhere else (Stats): which arm of which type ran, with which include_p0 and
which outcome of the predicate; and how many bits l and r needed.

geometric_count is independent of all of the above: the signed number of crossings of the curve with the ray from p
towards +x, from the roots of y(t) = py in exact arithmetic on a + b sqrt(d)."""
from collections import Counter
from fractions import Fraction

(X_AXIS, BALANCE, UP_STRAIGHT, UP_NORMAL, UP_U, UP_INV_U, DOWN_STRAIGHT, DOWN_NORMAL, DOWN_INV_U, DOWN_U) = range(10)
TYPE_NAMES = ("x_axis", "balance", "up_straight", "up_normal", "up_u", "up_inv_u",
              "down_straight", "down_normal", "down_inv_u", "down_u")
OVERFLOW_COLOUR = 150
BIG_BITS = 100


class Stats:
    """arms[(type name, arm, include_p0, predicate outcome or None)], solver[(predicate, outcome)], the widest l and r
    compared, and eq_big[(predicate, outcome)]: the l == r decisions taken on operands of more than BIG_BITS bits"""

    def __init__(self):
        self.arms = Counter()
        self.solver = Counter()
        self.eq_big = Counter()
        self.bits_l = 0
        self.bits_r = 0
        self.last = None

    def compared(self, l, r):
        self.bits_l = max(self.bits_l, l.bit_length())
        self.bits_r = max(self.bits_r, r.bit_length())

    def bits(self):
        return max(self.bits_l, self.bits_r)

    def merge(self, other):
        self.arms.update(other.arms)
        self.solver.update(other.solver)
        self.eq_big.update(other.eq_big)
        self.bits_l = max(self.bits_l, other.bits_l)
        self.bits_r = max(self.bits_r, other.bits_r)
        return self


def sgn(v):
    return (v > 0) - (v < 0)


# ---- rules 1 and 2 -------------------------------------------------------------------------------------------------
def curve_type(p0, p1, p2):
    if p0[1] == p2[1]:
        return X_AXIS if p1[1] == p0[1] else BALANCE
    up = p0[1] < p2[1]
    if abs(p0[0] + p2[0] - 2 * p1[0]) <= 1 and abs(p0[1] + p2[1] - 2 * p1[1]) <= 1:
        return UP_STRAIGHT if up else DOWN_STRAIGHT
    if min(p0[1], p2[1]) <= p1[1] <= max(p0[1], p2[1]):
        return UP_NORMAL if up else DOWN_NORMAL
    if up:
        return UP_U if p1[1] < p0[1] else UP_INV_U
    return DOWN_INV_U if p1[1] > p0[1] else DOWN_U


def scaled(glyph, K):
    return [[(K * x, K * y) for (x, y) in c] for c in glyph]


def curves_of(glyph, K=1):
    """every curve of the K-times scaled glyph, contours back to back: (type, include_p0, p0, p1, p2)"""
    out = []
    for pts in scaled(glyph, K):
        n = len(pts) // 2
        for k in range(n):
            p0, p1, p2 = pts[2 * k], pts[2 * k + 1], pts[2 * k + 2]
            j = (k - 1) % n                                   # the previous curve of the contour, wrapping
            q0, q1 = pts[2 * j], pts[2 * j + 1]
            prev_end = 2 * sgn(p0[1] - q1[1]) + sgn(p0[1] - q0[1])
            curr_start = 2 * sgn(p1[1] - p0[1]) + sgn(p2[1] - p0[1])
            inc = curr_start != 0 and (prev_end == 0 or (prev_end > 0) != (curr_start < 0))
            out.append((curve_type(p0, p1, p2), bool(inc), p0, p1, p2))
    return out


def glyph_info(glyph, K=1):
    cs = curves_of(glyph, K)
    return [c[0] for c in cs], [int(c[1]) for c in cs]


# ---- rule 3 --------------------------------------------------------------------------------------------------------
def _terms(p, p0, p1, p2):
    ay, by, cy = p0[1] + p2[1] - 2 * p1[1], 2 * (p1[1] - p0[1]), p0[1] - p[1]
    ax, bx, cx = p0[0] + p2[0] - 2 * p1[0], 2 * (p1[0] - p0[0]), p0[0] - p[0]
    dy = by * by - 4 * ay * cy
    abxy = ax * by - ay * bx
    tmp = 2 * ay * (ax * cy - ay * cx) - by * abxy
    return dy, abxy, tmp


def _order(l, r):
    return "l<r" if l < r else ("l==r" if l == r else "l>r")


def _note(stats, name, outcome, l=None, r=None):
    if stats is not None:
        stats.solver[(name, outcome)] += 1
        stats.last = outcome
        if l is not None:
            stats.compared(l, r)
            if l == r and max(l.bit_length(), r.bit_length()) > BIG_BITS:
                stats.eq_big[(name, outcome)] += 1


def two_roots(p, p0, p1, p2, stats=None):
    dy, abxy, tmp = _terms(p, p0, p1, p2)
    if dy <= 0:
        _note(stats, "solve2", "dy<=0")
        return 0
    if abxy == 0:
        _note(stats, "solve2", "abxy==0")
        return 0
    s = sgn(abxy)
    if tmp == 0:
        _note(stats, "solve2", "tmp==0")
        return s
    l, r = dy * abxy * abxy, tmp * tmp
    _note(stats, "solve2", ("tmp>0," if tmp > 0 else "tmp<0,") + _order(l, r), l, r)
    if tmp > 0:
        return 0 if l < r else s
    return 0 if l <= r else s


def one_root(p, p0, p1, p2, tilt_up, stats=None):
    dy, abxy, tmp = _terms(p, p0, p1, p2)
    if dy == 0:
        _note(stats, "solve1", "dy==0")
        return False
    if abxy == 0:
        _note(stats, "solve1", "abxy==0,tmp<=0" if tmp <= 0 else "abxy==0,tmp>0")
        return tmp <= 0
    if (abxy > 0) != tilt_up:
        if tmp <= 0:
            _note(stats, "solve1", "A,tmp<=0")
            return True
        l, r = dy * abxy * abxy, tmp * tmp
        _note(stats, "solve1", "A," + _order(l, r), l, r)
        return l >= r
    if tmp >= 0:
        _note(stats, "solve1", "B,tmp>=0")
        return False
    l, r = dy * abxy * abxy, tmp * tmp
    _note(stats, "solve1", "B," + _order(l, r), l, r)
    return l <= r


# ---- rule 4 --------------------------------------------------------------------------------------------------------
def curve_winding(ct, inc, p0, p1, p2, p, stats=None):
    """(winding contribution, arm or None) of one curve of the scaled glyph at p"""
    px, py = p
    if stats is not None:
        stats.last = None
    w, arm = 0, None
    if ct == X_AXIS:
        return 0, None
    if ct == BALANCE:
        if inc and py == p0[1]:
            arm = "row"
            if px < p0[0]:
                w = 1 if p1[1] < p0[1] else -1
        elif (p1[1] >= p0[1]) == (py >= p0[1]):
            arm = "two_roots"
            w = two_roots(p, p0, p1, p2, stats)
    elif ct in (UP_STRAIGHT, DOWN_STRAIGHT, UP_NORMAL, DOWN_NORMAL):
        lo, hi = min(p0[1], p2[1]), max(p0[1], p2[1])
        if lo < py < hi:
            arm = "inside"
        elif inc and py == p0[1]:
            arm = "at_p0"
        if arm:
            up = ct in (UP_STRAIGHT, UP_NORMAL)
            if ct in (UP_STRAIGHT, DOWN_STRAIGHT):
                v1, v2 = (py - p0[1]) * (p2[0] - p0[0]), (px - p0[0]) * (p2[1] - p0[1])
                hit = v1 >= v2 if up else v1 <= v2
            else:
                hit = one_root(p, p0, p1, p2, up, stats)
            if hit:
                w = -1 if up else 1
    elif ct in (UP_INV_U, DOWN_U):
        up = ct == UP_INV_U
        beyond = py > p2[1] if up else py < p2[1]
        if min(p0[1], p2[1]) < py < max(p0[1], p2[1]):
            arm = "inside"
        elif py == p2[1]:
            arm = "at_p2"
        elif py == p0[1] and inc:
            arm = "at_p0"
        elif beyond:
            arm = "two_roots"
        if arm == "two_roots":
            w = two_roots(p, p0, p1, p2, stats)
        elif arm and one_root(p, p0, p1, p2, up, stats):
            w = -1 if up else 1
    else:
        assert ct in (UP_U, DOWN_INV_U)
        up = ct == UP_U
        beyond = py < p0[1] if up else py > p0[1]
        if min(p0[1], p2[1]) < py < max(p0[1], p2[1]):
            arm = "inside"
            if one_root(p, p0, p1, p2, up, stats):
                w = -1                                   # for down_inv_u too: the reference's own sign, kept
        elif py == p0[1]:
            cross = one_root(p, p0, p1, p2, up, stats)
            side = px <= p0[0] if up else px > p0[0]
            if inc and cross != side:
                arm = "at_p0_contrib"
                w = (-1 if cross else 1) if up else (1 if cross else -1)
            else:
                arm = "at_p0_none"
        elif beyond:
            arm = "two_roots"
            w = two_roots(p, p0, p1, p2, stats)
    if stats is not None and arm is not None:
        stats.arms[(TYPE_NAMES[ct], arm, inc, stats.last)] += 1
    return w, arm


# ---- rule 5 --------------------------------------------------------------------------------------------------------
def winding_at(curves, p, stats=None):
    w = 0
    for (ct, inc, p0, p1, p2) in curves:
        w += curve_winding(ct, inc, p0, p1, p2, p, stats)[0]
    return w


def winding_in_glyph(glyph, queries, stats=None):
    """the windings of the unscaled glyph at a list of points"""
    cs = curves_of(glyph, 1)
    return [winding_at(cs, (int(x), int(y)), stats) for (x, y) in queries]


def exact_lattice(glyph, K, x0, y0, w, h, stats=None):
    """rows j of the windings at (x0 + i, y0 - j) of the K-times scaled glyph"""
    cs = curves_of(glyph, K)
    return [[winding_at(cs, (x0 + i, y0 - j), stats) for i in range(w)] for j in range(h)]


def box_of(glyph):
    """(x_min, y_min, x_max, y_max) over every point, control points included"""
    xs = [x for c in glyph for (x, _) in c]
    ys = [y for c in glyph for (_, y) in c]
    return (min(xs), min(ys), max(xs), max(ys)) if xs else (0, 0, 0, 0)


def winding_lattice(glyph, box, stats=None):
    """the debug image's lattice: the box with a border of one unit, K = 1"""
    return exact_lattice(glyph, 1, box[0] - 1, box[3] + 1, box[2] - box[0] + 3, box[3] - box[1] + 3, stats)


def inside_counts(lat, n):
    """per pixel, the number of its n x n lattice points with a non-zero winding"""
    h_px, w_px = len(lat) // n, len(lat[0]) // n
    return [[sum(lat[y * n + j][x * n + i] != 0 for j in range(n) for i in range(n)) for x in range(w_px)]
            for y in range(h_px)]


def round_half_up_255(k, n):
    return (2 * 255 * k + n * n) // (2 * n * n)


def exact_coverage(glyph, K, x0, y0, w_px, h_px, n, stats=None):
    """-> (coverage rows, inside-count rows)"""
    counts = inside_counts(exact_lattice(glyph, K, x0, y0, w_px * n, h_px * n, stats), n)
    return [[round_half_up_255(k, n) for k in row] for row in counts], counts


def debug_colour(v, scale, overflow=OVERFLOW_COLOUR):
    c = min(abs(v) * scale, 65535)
    main = min(c, 255)
    sub = 0 if c == main else overflow
    return (sub, sub, main) if v > 0 else (main, sub, sub)


def debug_render(glyph, box, scale, lat=None):
    """rows of RGB triples: the lattice of winding_lattice coloured, then every curve's points marked"""
    lat = winding_lattice(glyph, box) if lat is None else lat
    img = [[debug_colour(v, scale) for v in row] for row in lat]
    for c in glyph:
        for k in range(len(c) // 2):
            for (x, y), mark in ((c[2 * k], (255, 255, 0)), (c[2 * k + 1], (0, 255, 255))):
                img[box[3] - y + 1][x - box[0] + 1] = mark
    return img


# ---- the independent count -------------------------------------------------------------------------------------------
def _sign_surd(a, b, d):
    """sign of a + b sqrt(d) for rational a, b and an integer d >= 0"""
    sa, sb = sgn(a), sgn(b) * (d > 0)
    if sa == 0 or sb == 0 or sa == sb:
        return sa or sb
    return sa * sgn(a * a - b * b * d)


def geometric_count(p0, p1, p2, p):
    """- sum of sign(y'(t)) over the roots t in (0, 1) of y(t) = py with x(t) > px, or None where p is not generic for
    the curve: py on the height of an end point, a double root, or p on the curve.  p1 may be rational (a chord's
    middle)."""
    px, py = p
    if py == p0[1] or py == p2[1]:
        return None
    ay, by, cy = p0[1] + p2[1] - 2 * p1[1], 2 * (p1[1] - p0[1]), p0[1] - py
    ax, bx, cx = p0[0] + p2[0] - 2 * p1[0], 2 * (p1[0] - p0[0]), p0[0] - px
    if ay == 0:
        if by == 0:
            return 0                              # a horizontal run on another height
        t = Fraction(-cy) / by
        if not 0 < t < 1:
            return 0
        s = sgn(cx + bx * t + ax * t * t)
        if s == 0:
            return None
        return -sgn(by) if s > 0 else 0
    d = by * by - 4 * ay * cy
    if d == 0:
        return None
    if d < 0:
        return 0
    total = 0
    u = Fraction(-by) / (2 * ay)
    for s in (1, -1):
        v = Fraction(s) / (2 * ay)                  # t = u + v sqrt(d), y'(t) = 2 ay t + by = s sqrt(d)
        if _sign_surd(u, v, d) <= 0 or _sign_surd(u - 1, v, d) >= 0:
            continue
        side = _sign_surd(cx + bx * u + ax * (u * u + v * v * d), bx * v + 2 * ax * u * v, d)
        if side == 0:
            return None
        if side > 0:
            total -= s
    return total

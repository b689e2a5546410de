"""CPU checks of the exact-integer path's Python-int reference (tests/exact_ref.py) and of the cases built on it
(tests/exact_cases.py): the cases reach every arm of the rules, every outcome of the two predicates and the top of the
128-bit range; the reference agrees with an independent crossing count except where the rules themselves do not; and
the reference equals the C oracle on every case.  tests/test_gpu_exact.py holds the device to the same answers.

Predicate outcomes.  An exhaustive search over p0, p1, p2, p in [-4, 4]^2 with include_p0 both ways (43 million curve
and point pairs through exact_ref.curve_winding) reached all 9 outcomes of two_roots and all 11 of one_root, so none
is listed as unreachable.  Two are reachable from one place only, which the counters confirm here: one_root's
dy == 0 needs p on the height of the parabola's vertex, and the arms call it on the open side of the vertex except for a
normal curve that starts flat (p1y == p0y) queried at_p0; and within up_u / down_inv_u at_p0 the outcome decides
between "contribution" and "none", so each of those two arms sees only part of the outcomes."""
import random
from collections import Counter

import numpy as np
import pytest

import exact_cases as EC
import exact_ref as R

NEEDS_P0 = {"row", "at_p0", "at_p0_contrib"}
ARMS = ([("balance", a) for a in ("row", "two_roots")]
        + [(t, a) for t in ("up_straight", "up_normal", "down_straight", "down_normal") for a in ("inside", "at_p0")]
        + [(t, a) for t in ("up_inv_u", "down_u") for a in ("inside", "at_p0", "at_p2", "two_roots")]
        + [(t, a) for t in ("up_u", "down_inv_u") for a in ("inside", "at_p0_contrib", "at_p0_none", "two_roots")])
SOLVE2 = ["dy<=0", "abxy==0", "tmp==0"] + [s + o for s in ("tmp>0,", "tmp<0,") for o in ("l<r", "l==r", "l>r")]
SOLVE1 = (["dy==0", "abxy==0,tmp<=0", "abxy==0,tmp>0", "A,tmp<=0", "B,tmp>=0"]
          + [s + o for s in ("A,", "B,") for o in ("l<r", "l==r", "l>r")])
EQUALITIES = [("solve2", "tmp>0,l==r"), ("solve2", "tmp<0,l==r"), ("solve1", "A,l==r"), ("solve1", "B,l==r")]


@pytest.fixture(scope="module")
def stats():
    return EC.all_stats()


def test_every_arm_runs(stats):
    hits = Counter()
    for (ty, arm, inc, _), n in stats.arms.items():
        hits[(ty, arm, inc)] += n
    assert {(t, a) for (t, a, _) in hits} == set(ARMS)
    for (ty, arm) in ARMS:
        for inc in ((True,) if arm in NEEDS_P0 else (True, False)):
            assert hits[(ty, arm, inc)] >= 20, (ty, arm, inc, hits[(ty, arm, inc)])
        if arm in NEEDS_P0:
            assert hits[(ty, arm, False)] == 0


def test_every_predicate_outcome_runs(stats):
    assert {k for k in stats.solver} == {("solve2", o) for o in SOLVE2} | {("solve1", o) for o in SOLVE1}
    for k, n in stats.solver.items():
        assert n >= 20, (k, n)
    where = {(ty, arm) for (ty, arm, _, out) in stats.arms if out == "dy==0"}
    assert where == {("up_normal", "at_p0"), ("down_normal", "at_p0")}


def test_small_tier_has_the_shapes_it_names():
    one_curve = flat_before = d2_one = 0
    for g in EC.small_glyphs():
        one_curve += sum(len(c) == 3 for c in g)
        for c in g:
            n = len(c) // 2
            for k in range(n):
                p0, p1, p2 = c[2 * k], c[2 * k + 1], c[2 * k + 2]
                q0, q1 = c[2 * ((k - 1) % n)], c[2 * ((k - 1) % n) + 1]
                flat_before += q0[1] == q1[1] == p0[1] and (p1[1] != p0[1] or p2[1] != p0[1])
                d2 = (abs(p0[0] + p2[0] - 2 * p1[0]), abs(p0[1] + p2[1] - 2 * p1[1]))
                d2_one += max(d2) == 1 and p0[1] != p2[1]
        t1, t2 = R.glyph_info(g, 1)[0], R.glyph_info(g, 2)[0]
        assert all((a == b) or a in (R.UP_STRAIGHT, R.DOWN_STRAIGHT) for a, b in zip(t1, t2))
    assert one_curve >= 5 and flat_before >= 5 and d2_one >= 20, (one_curve, flat_before, d2_one)
    # straight at K = 1 only: the scaled glyph is what gets classified
    g = [[(0, 0), (2, 3), (5, 7), (1, 4), (0, 0)]]
    assert R.glyph_info(g, 1)[0][0] == R.UP_STRAIGHT and R.glyph_info(g, 2)[0][0] == R.UP_NORMAL


def test_limit_tier_fills_the_range():
    st = EC.tier("limit")[1]
    assert st["limit_k1"].bits() >= 100, st["limit_k1"].bits()
    assert st["limit_k8"].bits() >= 118, st["limit_k8"].bits()
    assert max(s.bits() for s in st.values()) <= 127          # what the signed 128-bit type of the device can hold
    big = Counter()
    for s in st.values():
        big.update(s.eq_big)
    for k in EQUALITIES:
        assert big[k] >= 5, (k, big[k])
    for g in EC.limit_glyphs():
        assert all(-32767 <= v <= 32767 for c in g for pt in c for v in pt)
    flat = [v for g in EC.limit_glyphs() for c in g for pt in c for v in pt]
    assert 32767 in flat and -32767 in flat and 32752 in flat and -32752 in flat


def test_many_tier_sizes():
    assert sorted(EC.many_glyphs()) == [255, 256, 257, 513]
    for n, g in EC.many_glyphs().items():
        assert sum(len(c) // 2 for c in g) == n
    lens = sorted({len(j.args[0]) for j in EC.tier("many")[0] if j.kind == "query"})
    assert lens == [1, 255, 256, 257]
    # the windings are not the work of the first 256 curves alone: the staging loop's later chunks matter
    for n, g in EC.many_glyphs().items():
        if n > 256:
            lat = next(j for j in EC.tier("many")[0] if j.kind == "lattice" and j.glyph is g)
            cs = R.curves_of(g, 1)[:256]
            K, x0, y0, w, h = lat.args
            head = [[R.winding_at(cs, (x0 + i, y0 - j)) for i in range(w)] for j in range(h)]
            assert not np.array_equal(np.array(head), lat.expect)


def test_coverage_counts():
    seen = {n: set() for n in range(1, 9)}
    for j in EC.tier("coverage")[0]:
        if j.extra is not None:
            n = j.args[5]
            seen[n].update(k for row in j.extra for k in row)
            assert j.args[3] * n <= 64 and j.args[4] * n <= 64
    for n, ks in seen.items():
        assert 0 in ks and n * n in ks
        if n <= 4:
            assert ks == set(range(n * n + 1)), (n, sorted(ks))
        else:
            assert len(ks - {0, n * n}) >= 20, (n, sorted(ks))
    assert 2 in seen[2] and R.round_half_up_255(2, 2) == 128
    assert [R.round_half_up_255(k, 2) for k in range(5)] == [0, 64, 128, 191, 255]


def test_colour_cases():
    jobs = EC.tier("colour")[0]
    lat = next(j for j in jobs if j.kind == "wlattice").expect
    assert set(range(-5, 6)) <= set(np.unique(lat).tolist())
    assert [j.args[0] for j in jobs if j.kind == "debug"] == [1, 63, 64, 85, 86, 255]
    assert R.debug_colour(4, 64) == (150, 150, 255) and R.debug_colour(4, 63) == (0, 0, 252)
    assert R.debug_colour(-3, 85) == (255, 0, 0) and R.debug_colour(-3, 86) == (255, 150, 150)
    assert R.debug_colour(0, 255) == (0, 0, 0) and R.debug_colour(-32768, 255) == (255, 150, 150)


def test_reference_is_the_crossing_count_but_for_its_known_rules():
    """the per-curve winding against -sum sign(y') over the crossings right of p, on at least 100 000 generic (curve,
    point) pairs.  Two rules differ from the count and are kept as the reference has them:
      1. down_inv_u's inside arm adds -1 where the count is +1;
      2. a normal curve that is linear in y (ay == 0) has abxy = ax by, tmp = -ax by^2 and dy = by^2, so l == r and
         tmp's sign is ax's alone: one_root says "crossing" wherever p is, and the rule differs from the count where the
         curve is left of p.
    A straight type is its chord (rule 4), so its count is taken on the chord and must agree everywhere.  Found while
    writing this: against the parabola itself a straight curve with a second difference of +-1 differs at a few lattice
    points between chord and curve (48 of 44 690 such pairs in a run of 200 000) — the definition of the type (DESIGN.md
    section 6), not a misreading; it is counted here too, and must not occur with a second difference of 0."""
    from fractions import Fraction
    rng = random.Random(0x5EED0400)
    pairs = 0
    inv_u, lin_y, chord = Counter(), Counter(), Counter()
    other = []
    while pairs < 120000:
        a = (rng.randint(-12, 12), rng.randint(-12, 12))
        b = (rng.randint(-12, 12), rng.randint(-12, 12))
        c = EC._control(rng, a, b, 12)
        ct = R.curve_type(a, c, b)
        inc = rng.random() < 0.5
        straight = ct in (R.UP_STRAIGHT, R.DOWN_STRAIGHT)
        mid = (Fraction(a[0] + b[0], 2), Fraction(a[1] + b[1], 2)) if straight else c
        bent = straight and (a[0] + b[0] != 2 * c[0] or a[1] + b[1] != 2 * c[1])
        for _ in range(6):
            p = (rng.randint(-14, 14), rng.randint(-14, 14))
            geo = R.geometric_count(a, mid, b, p)
            if geo is None:
                continue
            pairs += 1
            ref, arm = R.curve_winding(ct, inc, a, c, b, p)
            if ct == R.DOWN_INV_U and arm == "inside":
                assert ref == -geo and geo in (0, 1), (a, c, b, p, ref, geo)
                inv_u[ref - geo] += 1
            elif ct in (R.UP_NORMAL, R.DOWN_NORMAL) and a[1] + b[1] - 2 * c[1] == 0 and arm == "inside":
                want = -1 if ct == R.UP_NORMAL else 1
                assert ref == want and geo in (0, want), (a, c, b, p, ref, geo)
                lin_y[ref - geo] += 1
            elif ref != geo:
                other.append((R.TYPE_NAMES[ct], arm, a, c, b, p, ref, geo))
            if straight:
                true = R.geometric_count(a, c, b, p)
                if true is not None:
                    chord[(bent, true == ref)] += 1
    assert not other, (len(other), other[:10])
    assert set(inv_u) == {0, -2} and inv_u[-2] >= 100, inv_u
    assert set(lin_y) == {0, -1, 1} and lin_y[-1] >= 20 and lin_y[1] >= 20, lin_y
    assert chord[(False, False)] == 0 and chord[(False, True)] >= 1000, chord
    assert chord[(True, False)] > 0 and chord[(True, True)] >= 1000, chord


def _fr_glyph(cache, g):
    if id(g) not in cache:
        cache[id(g)] = EC.to_fr(g)
    return cache[id(g)]


@pytest.mark.parametrize("name", EC.TIERS)
def test_reference_equals_oracle(oracle, name):
    cache = {}
    try:
        for j in EC.tier(name)[0]:
            g = _fr_glyph(cache, j.glyph)
            if j.kind == "info":
                ct, ip = oracle.glyph_info(g)
                assert np.array_equal(ct, j.expect[0]) and np.array_equal(ip, j.expect[1]), j
            elif j.kind == "query":
                assert np.array_equal(oracle.winding_in_glyph(g, j.args[0]), j.expect), j
            elif j.kind == "wlattice":
                assert np.array_equal(oracle.winding_lattice(g), j.expect), j
            elif j.kind == "lattice":
                assert np.array_equal(oracle.exact_lattice(g, *j.args), j.expect), j
            elif j.kind == "coverage":
                assert np.array_equal(oracle.exact_coverage(g, *j.args), j.expect), j
            else:
                assert j.kind == "debug"
                assert np.array_equal(oracle.glyph_debug_render(g, j.args[0]), j.expect), j
        if name == "colour":
            for v in list(range(-7, 8)) + [-32768, 32767, 257, -258]:
                for s in EC.COLOUR_SCALES:
                    assert oracle.winding_rgb(v, s, R.OVERFLOW_COLOUR) == R.debug_colour(v, s), (v, s)
    finally:
        oracle.diag_reset()           # the oracle's counters are process-wide: later tests expect 0

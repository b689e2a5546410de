"""The numpy / Python-int twin of fr_layer_paint (tests/layer_paint_ref.py) against a brute force in exact fractions, and the
consequences the header states, on the CPU.  tests/test_gpu_layer_paint.py then holds the GPU to the twin byte for byte."""
import math
from fractions import Fraction

import numpy as np
import pytest

import layer_paint_ref as pr
import layer_rects_ref as rr
from layer_gpu import premultiplied

STOP_LISTS = {
    "one": [(30000, (9, 8, 7, 200))],
    "two_full_range": [(0, (255, 0, 0, 255)), (65536, (0, 0, 255, 255))],
    "two_inside": [(16000, (255, 0, 0, 255)), (48031, (0, 0, 255, 0))],
    "eight": [(0, (255, 0, 0, 255)), (100, (0, 255, 0, 0)), (9000, (0, 0, 255, 255)), (9000, (255, 255, 0, 128)), (30001, (1, 2, 3, 4)),
              (30002, (250, 251, 252, 253)), (65535, (0, 0, 0, 0)), (65536, (255, 255, 255, 255))],
    "hard_edges_only": [(32768, (255, 0, 0, 255)), (32768, (0, 255, 0, 255)), (32768, (0, 0, 255, 77))],
    "all_at_0": [(0, (1, 2, 3, 4)), (0, (5, 6, 7, 8))],
    "all_at_65536": [(65536, (1, 2, 3, 4)), (65536, (5, 6, 7, 8))],
    "odd_width": [(5, (0, 0, 0, 0)), (65534, (255, 254, 1, 255))],
}


def _exact_colour(stops, q):
    """the gradient at position q as exact fractions: before the first stop its colour, from the last stop on its colour,
    between two stops the straight line; of several stops at one offset the last one counts from there on"""
    if q < stops[0][0]:
        return [Fraction(v) for v in stops[0][1]]
    at = [j for j, s in enumerate(stops) if s[0] <= q][-1]
    if at == len(stops) - 1:
        return [Fraction(v) for v in stops[at][1]]
    (o0, c0), (o1, c1) = stops[at], stops[at + 1]
    return [c0[c] + Fraction((c1[c] - c0[c]) * (q - o0), o1 - o0) for c in range(4)]


@pytest.mark.parametrize("name", sorted(STOP_LISTS))
def test_table_is_the_exact_gradient_rounded_half_up(name):
    stops = STOP_LISTS[name]
    G = pr.table(stops)
    assert G.shape == (1024, 4) and G.min() >= 0 and G.max() <= 255
    for k in range(1024):
        exact = _exact_colour(stops, 64 * k + 32)
        assert [int(v) for v in G[k]] == [math.floor(e + Fraction(1, 2)) for e in exact], (name, k)


def test_table_edges():
    G = pr.table(STOP_LISTS["hard_edges_only"])
    assert (G[:512] == (255, 0, 0, 255)).all() and (G[512:] == (0, 0, 255, 77)).all()      # q = 32800 is the first at or past 32768
    assert (pr.table(STOP_LISTS["one"]) == (9, 8, 7, 200)).all()
    assert (pr.table(STOP_LISTS["all_at_0"]) == (5, 6, 7, 8)).all() and (pr.table(STOP_LISTS["all_at_65536"]) == (1, 2, 3, 4)).all()
    G = pr.table(STOP_LISTS["two_full_range"])
    assert tuple(G[0]) == (255, 0, 0, 255) and tuple(G[1023]) == (0, 0, 255, 255) and (np.diff(G[:, 2]) >= 0).all() and (G[:, 0] + G[:, 2] == 255).all()
    G = pr.table(STOP_LISTS["eight"])
    # q = 8992 and 9056 around the hard edge at 9000: 255 * 8892 / 8900 = 254.8; 255 - 254 * 56 / 21001 = 254.3, 128 - 124 * 56 / 21001 = 127.7
    assert tuple(G[140]) == (0, 0, 255, 255) and tuple(G[141]) == (254, 254, 0, 128)


def test_rdiv_floors_for_either_sign():
    for n in range(-40, 41):
        for d in (1, 2, 3, 7, 8):
            assert pr.rdiv(n, d) == math.floor(Fraction(n, d) + Fraction(1, 2)), (n, d)


def _random_linear(rng):
    while True:
        x0, y0, x1, y1 = (int(v) for v in rng.integers(-2 ** 26, 2 ** 26 + 1, 4))
        if rng.integers(0, 3) == 0:                            # short ones too: down to a pixel
            x1, y1 = x0 + int(rng.integers(-300, 301)), y0 + int(rng.integers(-300, 301))
        if max(abs(x1), abs(y1)) <= 2 ** 26 and (x1 - x0) ** 2 + (y1 - y0) ** 2 >= 4096:
            return x0, y0, x1, y1


def test_linear_t_is_within_1_of_the_exact_projection():
    rng = np.random.default_rng(71)
    worst, bits = 0, 0
    for _ in range(3000):
        x0, y0, x1, y1 = _random_linear(rng)
        dx, dy = x1 - x0, y1 - y0
        c = pr.linear_coefficients(x0, y0, x1, y1)
        for X, Y in [(0, 0), (32767, 32767), (32767, 0), (0, 32767)] + [tuple(int(v) for v in rng.integers(0, 32768, 2)) for _ in range(4)]:
            exact = Fraction((64 * X + 32 - x0) * dx + (64 * Y + 32 - y0) * dy, dx * dx + dy * dy)
            worst = max(worst, abs(pr.linear_t(c, X, Y) - math.floor(65536 * exact)))
            bits = max(bits, abs(c[0] + X * c[1] + Y * c[2]).bit_length())
    assert worst <= 1 and bits <= 60, (worst, bits)


def test_linear_t_sum_stays_below_2_60_at_the_limits():
    for x0, y0, x1, y1 in [(-2 ** 26, -2 ** 26, -2 ** 26 + 64, -2 ** 26), (2 ** 26, 2 ** 26, 2 ** 26 - 46, 2 ** 26 - 45), (-2 ** 26, 2 ** 26, -2 ** 26, 2 ** 26 - 64)]:
        c = pr.linear_coefficients(x0, y0, x1, y1)
        for X in (0, 2 ** 26 - 1):
            for Y in (0, 2 ** 26 - 1):
                assert abs(c[0] + X * c[1] + Y * c[2]) < 2 ** 60


def test_dyadic_linear_t_is_exact():
    for x0, y0, x1, y1 in [(0, 0, 4096, 0), (64, 64, 64 + 2048, 64 + 2048), (100, -7, 100, -7 - 64), (4160, 4160, 64, 64)]:
        dx, dy = x1 - x0, y1 - y0
        c = pr.linear_coefficients(x0, y0, x1, y1)
        for X in range(-3, 200, 7):
            for Y in range(-3, 90, 5):
                assert pr.linear_t(c, X, Y) == math.floor(65536 * Fraction((64 * X + 32 - x0) * dx + (64 * Y + 32 - y0) * dy, dx * dx + dy * dy))


def test_radial_t_is_within_its_bound():
    rng = np.random.default_rng(72)
    for k in range(3000):
        r = int(rng.integers(64, 2 ** 26 + 1)) if k % 3 else int(rng.integers(64, 6400))
        x0, y0 = (int(v) for v in rng.integers(-2 ** 26, 2 ** 26 + 1, 2))
        R = pr.radial_coefficient(r)
        for _ in range(4):
            X, Y = (int(v) for v in rng.integers(0, 2 ** 20, 2))
            ddx, ddy = 64 * X + 32 - x0, 64 * Y + 32 - y0
            if max(abs(ddx), abs(ddy)) >= 2 ** 27:
                continue
            exact = math.isqrt(65536 * 65536 * (ddx * ddx + ddy * ddy) // (r * r))         # floor(65536 dist / r)
            assert abs(pr.radial_t(x0, y0, R, X, Y) - exact) <= 1 + Fraction(4096, r), (x0, y0, r, X, Y)
    # the largest product: both distances just under 2^27 and the smallest radius
    assert pr.radial_t(-2 ** 26, -2 ** 26, pr.radial_coefficient(64), 2 ** 20 - 1, 2 ** 20 - 1) < 2 ** 38


def test_spreads_for_either_sign():
    for t in list(range(-140000, 140000, 331)) + [-131073, -131072, -131071, -65537, -65536, -65535, -1, 0, 1, 65535, 65536, 65537, 131071, 131072, -2 ** 59, 2 ** 59]:
        whole, frac = divmod(Fraction(t), 65536)               # floor and the rest in [0, 65536)
        assert pr.spread_u(t, pr.PAD) == (0 if t < 0 else 65535 if t > 65535 else t)
        assert pr.spread_u(t, pr.REPEAT) == frac
        assert pr.spread_u(t, pr.REFLECT) == (frac if whole % 2 == 0 else 65535 - frac)
        assert pr.spread_u(t, pr.REFLECT) == pr.spread_u(-1 - t, pr.REFLECT)           # a mirror between -1 and 0
    assert [pr.spread_u(t, pr.REPEAT) for t in (-1, -65536, -65537)] == [65535, 0, 65535]
    assert [pr.spread_u(t, pr.REFLECT) for t in (-1, -2, -65536, -65537, 65536, 131071, 131072)] == [0, 1, 65535, 65535, 65535, 0, 0]


TWO = STOP_LISTS["two_full_range"]


def test_consequence_4_moving_by_one_pixel():
    """dyadic linear gradients (TX, TY and T0 exact) and radial ones: geometry + (64, 64) and the position + (1, 1) move the
    image by one pixel"""
    rng = np.random.default_rng(73)
    image, layer = premultiplied(rng, (30, 70)), premultiplied(rng, (24, 60))
    for grad, moved in [((pr.LINEAR, pr.REFLECT, (64, 64, 64 + 2048, 64 + 2048), TWO), (pr.LINEAR, pr.REFLECT, (128, 128, 128 + 2048, 128 + 2048), TWO)),
                        ((pr.LINEAR, pr.REPEAT, (1000, 0, 1000 - 1024, 0), TWO), (pr.LINEAR, pr.REPEAT, (1064, 64, 1064 - 1024, 64), TWO)),
                        ((pr.RADIAL, pr.REPEAT, (1237, 911, 777, 0), TWO), (pr.RADIAL, pr.REPEAT, (1301, 975, 777, 0), TWO))]:
        for srgb in (False, True):
            a = pr.paint(image, layer, (0, 0, 60, 24), (2, 3), grad, srgb)
            b = pr.paint(np.roll(image, (1, 1), (0, 1)), layer, (0, 0, 60, 24), (3, 4), moved, srgb)
            assert np.array_equal(a[3:27, 2:62], b[4:28, 3:63]) and not np.array_equal(a, image)


def test_consequence_5_rows_and_symmetry():
    u = pr.parameter((pr.LINEAR, pr.PAD, (37, 500, 19001, 500), TWO), 0, 0, 300, 6)
    assert (u == u[0]).all() and len(set(u[0].tolist())) > 250
    for cx, cy, n in ((64 * 20 + 32, 64 * 15 + 32, 41), (64 * 20, 64 * 15, 40)):               # a pixel centre; a pixel corner
        for spread in (pr.PAD, pr.REPEAT, pr.REFLECT):
            u = pr.parameter((pr.RADIAL, spread, (cx, cy, 64 * 7 + 3, 0), TWO), 0, 0, n, n - 10)
            assert np.array_equal(u, u[::-1]) and np.array_equal(u, u[:, ::-1]) and u.min() != u.max()


def test_consequences_1_and_3():
    rng = np.random.default_rng(74)
    image, layer = premultiplied(rng, (20, 50)), premultiplied(rng, (20, 50))
    one = (pr.LINEAR, pr.PAD, (0, 0, 640, 0), [(123, (17, 250, 3, 180))])
    for srgb in (False, True):
        got = pr.paint(image, None, (0, 0, 30, 10), (7, 4), one, srgb)
        assert np.array_equal(got, rr.rects(image, [(64 * 7, 64 * 4, 64 * 37, 64 * 14, (17, 250, 3, 180))], srgb))
    grad = (pr.RADIAL, pr.REFLECT, (1600, 640, 900, 0), STOP_LISTS["eight"])
    out = pr.paint(np.zeros_like(image), layer, (0, 0, 50, 20), (0, 0), grad).astype(np.int64)
    assert (out[..., :3] <= out[..., 3:]).all() and out[..., 3].max() > 200                   # a valid premultiplied layer
    assert np.array_equal(out[layer[..., 3] == 0], np.zeros_like(out[layer[..., 3] == 0]))

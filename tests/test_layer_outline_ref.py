"""The numpy twin of fr_layer_outline (tests/layer_outline_ref.py) held to a brute-force loop over the header's definition in
Python ints, the disc weights to exact arithmetic for every radius, and the twin to the header's seven consequences.  No
GPU."""
import math
from fractions import Fraction

import numpy as np
import pytest

import layer_outline_ref as orf
import layer_shadow_ref as sr

KINDS = (orf.GROW, orf.RING, orf.INNER, orf.SHRINK)


def _m(x, y):
    return (x * y + 127) // 255


def _brute(a0, rho):
    """the four kinds on the window grown by R, pixel by pixel from the definition, in Python ints"""
    h, w = len(a0), len(a0[0])
    R = orf.reach(rho)

    def A0(u, v):
        return a0[v][u] if 0 <= u < w and 0 <= v < h else 0

    def G(A, u, v):
        return max(_m(A(u + i, v + j), orf.weight(rho, i, j)) for j in range(-R, R + 1) for i in range(-R, R + 1))

    out = [np.zeros((h + 2 * R, w + 2 * R), np.int64) for _ in KINDS]
    for v in range(-R, h + R):
        for u in range(-R, w + R):
            g, s = G(A0, u, v), 255 - G(lambda x, y: 255 - A0(x, y), u, v)
            for k, val in zip(KINDS, (g, g - A0(u, v), A0(u, v) - s, s)):
                out[k][v + R, u + R] = val
    return out


@pytest.mark.parametrize("shape", [(9, 12), (1, 1), (3, 8)], ids=lambda s: "%dx%d" % (s[1], s[0]))
def test_twin_is_the_definition(shape):
    rng = np.random.default_rng(shape[0] * 16 + shape[1])
    a0 = rng.integers(0, 256, shape)
    a0[rng.integers(0, 3, shape) == 0] = 255
    a0[rng.integers(0, 3, shape) == 0] = 0
    for rho in (0, 1, 8, 15, 16, 17, 40, 50):
        want = _brute(a0.tolist(), rho)
        got = orf.alpha_planes(a0, rho)
        for k in KINDS:
            assert np.array_equal(got[k], want[k]), (rho, k)
            assert got[k].min() >= 0 and got[k].max() <= 255


def test_weights_for_every_radius():
    """q is the floor of 256 times the distance; K is within 1.5 of 255 * clamp(rho / 16 + 1 - d, 0, 1) (one floor, then one
    rounding), compared without a square root: d < X is X > 0 and i^2 + j^2 < X^2; K(0, 0) = 255, the reach is R, K does not
    increase along a row and has the square's symmetries"""
    for rho in range(257):
        R = orf.reach(rho)
        K = orf.weights(rho)
        assert K.shape == (2 * R + 1, 2 * R + 1) and K[R, R] == 255
        assert np.array_equal(K, K.T) and np.array_equal(K, K[::-1]) and np.array_equal(K, K[:, ::-1])
        assert (np.diff(K[:, R:], axis=1) <= 0).all()
        assert K[R, 2 * R] > 0 or rho == 0                      # the reach is R, no less
        e = Fraction(rho, 16) + 1
        for j in range(0, R + 2):
            for i in range(j, R + 2):                            # one octant, and one ring beyond the table
                n = i * i + j * j
                q = math.isqrt(65536 * n)
                assert q * q <= 65536 * n < (q + 1) * (q + 1)
                k = orf.weight(rho, i, j)
                if i > R:
                    assert k == 0
                lo, hi = Fraction(2 * k - 3, 510), Fraction(2 * k + 3, 510)

                def d_below(X):
                    return X > 0 and n < X * X

                def d_above(X):
                    return X < 0 or n > X * X

                # c = clamp(e - d, 0, 1): lo < c < hi
                assert lo < 0 or (lo < 1 and d_below(e - lo)), (rho, i, j, k)
                assert hi > 1 or (hi > 0 and d_above(e - hi)), (rho, i, j, k)


def test_rim_offsets_are_few():
    """K is strictly between 0 and 255 on at most 6 offsets per side of any kernel row: the ramp is one pixel wide"""
    for rho in range(257):
        K = orf.weights(rho)
        R = orf.reach(rho)
        assert ((K[:, R + 1:] > 0) & (K[:, R + 1:] < 255)).sum(axis=1).max(initial=0) <= 6


def test_one_division_after_the_maximum():
    """m is monotone in the product, so the maximum of the raw products divided once is the maximum of the m's"""
    x = np.arange(255 * 255 + 1)
    assert (np.diff((x + 127) // 255) >= 0).all()


@pytest.fixture(scope="module")
def layer():
    rng = np.random.default_rng(23)
    a = rng.integers(0, 256, (11, 13, 1))
    a[rng.integers(0, 3, (11, 13, 1)) == 0] = 0
    a[rng.integers(0, 4, (11, 13, 1)) == 0] = 255
    return np.concatenate([rng.integers(0, 256, (11, 13, 3)) * a // 255, a], -1).astype(np.uint8)


WIN = (0, 0, 13, 11)


def _alpha(layer, size, offset, rho, kind, window=WIN):
    return orf.outline_rect(layer, window, size, offset, rho, kind, (255, 255, 255, 255))[..., 3].astype(np.int64)


def test_consequence_1_radius_0(layer):
    for srgb in (False, True):
        for colour in ((255, 255, 255, 255), (30, 144, 255, 200)):
            want = sr.shadow_rect(layer, WIN, (17, 15), (2, 2), 0, 0, 0, colour, srgb)
            assert np.array_equal(orf.outline_rect(layer, WIN, (17, 15), (2, 2), 0, orf.GROW, colour, srgb), want)
            assert np.array_equal(orf.outline_rect(layer, WIN, (17, 15), (2, 2), 0, orf.SHRINK, colour, srgb), want)
            for kind in (orf.RING, orf.INNER):
                assert not orf.outline_rect(layer, WIN, (17, 15), (2, 2), 0, kind, colour, srgb).any()


def test_consequence_2_an_impulse_gives_the_table():
    one = np.zeros((1, 1, 4), np.uint8)
    one[0, 0, 3] = 255
    for rho in (0, 1, 8, 16, 17, 100, 256):
        R = orf.reach(rho)
        got = _alpha(one, (2 * R + 5, 2 * R + 5), (R + 2, R + 2), rho, orf.GROW, (0, 0, 1, 1))
        want = np.zeros((2 * R + 5, 2 * R + 5), np.int64)
        want[2:2 * R + 3, 2:2 * R + 3] = orf.weights(rho)
        assert np.array_equal(got, want), rho


def test_consequence_3_whole_pixel_radii_move_an_edge():
    edge = np.zeros((9, 40, 4), np.uint8)
    edge[:, :10, 3] = 255
    edge[:, 10, 3] = 128
    for k in range(1, 17):
        for a in (edge, np.ascontiguousarray(edge.transpose(1, 0, 2))):
            w, h = a.shape[1], a.shape[0]
            got = _alpha(a, (w, h), (0, 0), 16 * k, orf.GROW, (0, 0, w, h))
            line = got[4] if a is edge else got[:, 4]
            assert line[:10 + k].tolist() == [255] * (10 + k) and line[10 + k] == 128 and not line[11 + k:40].any(), k
    hard = np.zeros((5, 12, 4), np.uint8)
    hard[:, :6, 3] = 255
    assert orf.weight(8, 1, 0) == 128
    assert _alpha(hard, (12, 5), (0, 0), 8, orf.GROW, (0, 0, 12, 5))[2].tolist() == [255] * 6 + [128] + [0] * 5


def test_consequence_4_the_sandwich_and_the_reach(layer):
    a0 = layer[..., 3].astype(np.int64)
    for rho in (1, 8, 16, 17, 40, 100, 128):
        R = orf.reach(rho)
        G, ring, inner, S = orf.alpha_planes(a0, rho)
        own = np.zeros_like(G)
        own[R:R + 11, R:R + 13] = a0
        assert (own <= G).all() and (G <= sr.alpha_plane(a0, R, 0, 0)).all()
        inside = np.zeros_like(G, bool)
        inside[R:R + 11, R:R + 13] = True
        assert not inner[~inside].any() and not S[~inside].any()
        # beyond the padded plane GROW is zero: a rectangle larger than the reach shows a frame of zeros
        more = _alpha(layer, (13 + 2 * R + 6, 11 + 2 * R + 6), (R + 3, R + 3), rho, orf.GROW)
        assert np.array_equal(more[3:-3, 3:-3], G) and more.sum() == G.sum()
        for off in ((-(13 + R), 0), (20 + R, 0), (0, -(11 + R)), (0, 20 + R)):
            for kind in KINDS:
                assert not _alpha(layer, (20, 20), off, rho, kind).any(), (rho, off, kind)
    # GROW is non-zero only within Chebyshev distance R of an inked pixel
    one = np.zeros((1, 1, 4), np.uint8)
    one[0, 0, 3] = 1
    assert _alpha(one, (9, 9), (4, 4), 40, orf.GROW, (0, 0, 1, 1)).astype(bool).sum() <= 49


def test_consequence_5_translation(layer):
    for kind in KINDS:
        base = orf.outline_rect(layer, WIN, (40, 40), (10, 10), 40, kind, (10, 200, 30, 180))
        for dx, dy in ((1, 0), (0, 1), (3, 2), (-1, -4)):
            got = orf.outline_rect(layer, WIN, (40, 40), (10 + dx, 10 + dy), 40, kind, (10, 200, 30, 180))
            assert np.array_equal(got, np.roll(base, (dy, dx), (0, 1))), (kind, dx, dy)


def test_consequence_6_the_eight_symmetries(layer):
    for kind in KINDS:
        for rho in (17, 56):
            base = orf.outline_rect(layer, (1, 2, 11, 8), (21, 18), (5, 5), rho, kind, (10, 200, 30, 180))
            for flip_x in (False, True):
                for flip_y in (False, True):
                    for swap in (False, True):
                        a, want = layer[2:10, 1:12], base
                        if flip_x:
                            a, want = a[:, ::-1], want[:, ::-1]
                        if flip_y:
                            a, want = a[::-1], want[::-1]
                        if swap:
                            a, want = a.transpose(1, 0, 2), want.transpose(1, 0, 2)
                        a = np.ascontiguousarray(a)
                        h, w = a.shape[:2]
                        got = orf.outline_rect(a, (0, 0, w, h), (w + 10, h + 10), (5, 5), rho, kind, (10, 200, 30, 180))
                        assert np.array_equal(got, want), (kind, rho, flip_x, flip_y, swap)


def test_consequence_7_monotone_in_the_radius(layer):
    a0 = layer[..., 3].astype(np.int64)
    P = 17
    prev = None
    for rho in range(0, 257, 3):
        R = orf.reach(rho)
        G, _, _, S = orf.alpha_planes(a0, rho)
        g = np.zeros((11 + 2 * P, 13 + 2 * P), np.int64)
        s = np.zeros_like(g)
        g[P - R:P + 11 + R, P - R:P + 13 + R] = G
        s[P - R:P + 11 + R, P - R:P + 13 + R] = S
        if prev is not None:
            assert (g >= prev[0]).all() and (s <= prev[1]).all(), rho
        prev = (g, s)


def test_the_window_is_all_that_is_read(layer):
    cut = np.zeros_like(layer)
    cut[3:8, 2:9] = layer[3:8, 2:9]
    for kind in (orf.GROW, orf.RING):
        a = orf.outline_rect(layer, (2, 3, 7, 5), (20, 20), (6, 6), 40, kind, (1, 2, 3, 255))
        b = orf.outline_rect(cut, (0, 0, 13, 11), (20, 20), (6 - 2, 6 - 3), 40, kind, (1, 2, 3, 255))
        assert np.array_equal(a, b)
    # INNER and SHRINK see the window's edge as an edge of the shape: a full window erodes from its border
    full = np.full((9, 9, 4), 255, np.uint8)
    assert np.array_equal(_alpha(full, (9, 9), (0, 0), 32, orf.SHRINK, (0, 0, 9, 9))[4], [0, 0, 255, 255, 255, 255, 255, 0, 0])
    assert np.array_equal(_alpha(full, (9, 9), (0, 0), 32, orf.INNER, (0, 0, 9, 9))[4], [255, 255, 0, 0, 0, 0, 0, 255, 255])

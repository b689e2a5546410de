"""The numpy twin of fr_layer_rects (tests/layer_rects_ref.py) held to a per-pixel brute force over the header's definition in
exact fractions (area and every rounding), and to the header's consequences 1, 2, 4, 5 and 6.  No GPU."""
from fractions import Fraction
from math import floor

import numpy as np
import pytest

import layer_ref as lr
import layer_rects_ref as rr
import layer_shadow_ref as sr


def _nearest(q):
    return floor(q + Fraction(1, 2))


def _brute(image, rows, srgb):
    """pixel by pixel: the area of the rectangle inside the pixel as a fraction, rounded to k; a; the composite"""
    D, E = lr.srgb_tables()
    out = [[[int(v) for v in px] for px in line] for line in image]
    h, w = image.shape[:2]
    for x0, y0, x1, y1, colour in rows:
        ex0, ey0, ex1, ey1 = (Fraction(int(v), 64) for v in (x0, y0, x1, y1))
        for Y in range(h):
            for X in range(w):
                area = max(Fraction(0), min(ex1, X + 1) - max(ex0, X)) * max(Fraction(0), min(ey1, Y + 1) - max(ey0, Y))
                k = _nearest(255 * area)
                a = _nearest(Fraction(k * int(colour[3]), 255))
                if a == 0:
                    continue
                d = out[Y][X]
                new = [0, 0, 0, a + _nearest(Fraction(d[3] * (255 - a), 255))]
                for c in range(3):
                    C = int(colour[c])
                    if srgb:
                        lin = _nearest(Fraction(int(D[C]) * a, 255)) + _nearest(Fraction(int(D[d[c]]) * (255 - a), 255))
                        new[c] = int(E[min(65535, lin)])
                    else:
                        new[c] = min(255, _nearest(Fraction(C * a, 255)) + _nearest(Fraction(d[c] * (255 - a), 255)))
                out[Y][X] = new
    return np.array(out, np.uint8)


def _premultiplied(rng, shape):
    a = rng.integers(0, 256, shape + (1,))
    a = np.where(rng.integers(0, 4, shape + (1,)) == 0, 255, a)
    return np.concatenate([rng.integers(0, 256, shape + (3,)) * a // 255, a], -1).astype(np.uint8)


def _random_rects(rng, n, w, h):
    rows = []
    for i in range(n):
        kind = i % 5
        x0, y0 = int(rng.integers(-100, 64 * w)), int(rng.integers(-100, 64 * h))
        if kind == 0:                                       # sub-pixel
            x1, y1 = x0 + int(rng.integers(1, 64)), y0 + int(rng.integers(1, 64))
        elif kind == 1:                                     # inverted or empty on one axis
            x1, y1 = x0 - int(rng.integers(0, 200)), y0 + int(rng.integers(1, 300))
        elif kind == 2:                                     # reaches far outside
            x0, y0, x1, y1 = -int(rng.integers(1, 2 ** 31)), y0, int(rng.integers(1, 2 ** 31)), y0 + int(rng.integers(1, 200))
        else:
            x1, y1 = x0 + int(rng.integers(1, 64 * w)), y0 + int(rng.integers(1, 64 * h))
        colour = tuple(int(v) for v in rng.integers(0, 256, 4))
        if i % 7 == 0:
            colour = colour[:3] + (255,)
        rows.append((x0, y0, x1, y1, colour))
    return rows


@pytest.mark.parametrize("srgb", [False, True], ids=["unorm", "srgb"])
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_twin_is_the_definition(seed, srgb):
    rng = np.random.default_rng(seed)
    w, h = 9, 7
    image = _premultiplied(rng, (h, w))
    rows = _random_rects(rng, 15, w, h) + [(64, 64, 192, 128, (9, 200, 30, 255)), (-2 ** 31, -2 ** 31, 2 ** 31 - 1, 2 ** 31 - 1, (1, 2, 3, 40))]
    got = rr.rects(image, rows, srgb)
    want = _brute(image, rows, srgb)
    assert np.array_equal(got, want), np.argwhere(got != want)[:4]
    assert not np.array_equal(got, image)


def test_every_coverage_value_is_the_rounded_area():
    for cx in range(65):
        for cy in range(65):
            k = int(rr.coverage((64, 128, 64 + cx, 128 + cy), 3, 4)[2, 1])
            assert k == _nearest(Fraction(255 * cx * cy, 4096)), (cx, cy)
    assert int(rr.coverage((0, 0, 64, 64), 1, 1)[0, 0]) == 255


@pytest.mark.parametrize("srgb", [False, True], ids=["unorm", "srgb"])
def test_consequence_1_an_aligned_opaque_rectangle_replaces(srgb):
    image = _premultiplied(np.random.default_rng(4), (6, 8))
    got = rr.rects(image, [(128, 64, 448, 320, (17, 250, 3, 255))], srgb)
    want = image.copy()
    want[1:5, 2:7] = (17, 250, 3, 255)
    assert np.array_equal(got, want)


def test_consequence_2_the_route_through_shadow_and_over():
    rng = np.random.default_rng(5)
    image = _premultiplied(rng, (7, 9))
    for x0, y0, x1, y1, colour in _random_rects(rng, 20, 9, 7):
        layer = np.zeros((7, 9, 4), np.uint8)
        layer[..., 3] = rr.coverage((x0, y0, x1, y1), 9, 7)
        tinted = sr.shadow_rect(layer, (0, 0, 9, 7), (9, 7), (0, 0), 0, 0, 0, colour)
        want = lr.over(tinted, image, 255)
        assert np.array_equal(rr.rects(image, [(x0, y0, x1, y1, colour)]), want), (x0, y0, x1, y1, colour)


@pytest.mark.parametrize("srgb", [False, True], ids=["unorm", "srgb"])
def test_consequence_4_moving_by_64_moves_by_a_pixel(srgb):
    image = np.zeros((8, 10, 4), np.uint8)
    image[:] = (40, 90, 20, 200)
    rect = (75, 130, 300, 260, (200, 10, 90, 180))
    at0 = rr.rects(image, [rect], srgb)
    for dx, dy in ((1, 0), (0, 1), (3, 2)):
        moved = rr.rects(image, [(rect[0] + 64 * dx, rect[1] + 64 * dy, rect[2] + 64 * dx, rect[3] + 64 * dy, rect[4])], srgb)
        want = image.copy()
        want[dy:, dx:] = at0[:8 - dy, :10 - dx]
        assert np.array_equal(moved, want), (dx, dy)
    assert not np.array_equal(at0, image)


@pytest.mark.parametrize("srgb", [False, True], ids=["unorm", "srgb"])
def test_consequence_5_symmetric_in_the_axes(srgb):
    rng = np.random.default_rng(6)
    image = _premultiplied(rng, (7, 9))
    rows = _random_rects(rng, 10, 9, 7)
    swapped = [(y0, x0, y1, x1, c) for x0, y0, x1, y1, c in rows]
    got = rr.rects(np.ascontiguousarray(image.transpose(1, 0, 2)), swapped, srgb)
    assert np.array_equal(got.transpose(1, 0, 2), rr.rects(image, rows, srgb))


def test_consequence_6_nothing_outside_the_bounding_boxes():
    rng = np.random.default_rng(7)
    image = rng.integers(0, 256, (7, 9, 4)).astype(np.uint8)        # not even premultiplied: those bytes are never looked at
    rows = [(70, 65, 130, 190, (1, 2, 3, 200)), (400, 300, 401, 301, (9, 9, 9, 255)), (-50, 385, 10, 500, (5, 6, 7, 90))]
    got = rr.rects(image, rows)
    inside = np.zeros((7, 9), bool)
    for r in rows:
        X0, Y0, X1, Y1 = rr.bounding_box(r, 9, 7)
        inside[Y0:Y1, X0:X1] = True
    assert rr.bounding_box(rows[0], 9, 7) == (1, 1, 3, 3) and rr.bounding_box(rows[2], 9, 7) == (0, 6, 1, 7)
    assert np.array_equal(got[~inside], image[~inside]) and not np.array_equal(got[inside], image[inside])
    assert rr.bounding_box((0, 0, 0, 64, None), 9, 7) is None and rr.bounding_box((64 * 9, 0, 64 * 10, 64, None), 9, 7) is None

"""The numpy twin of fr_layer_lcd (tests/layer_lcd_ref.py) held to a per-pixel brute force in plain Python ints, written a
second time from include/fr_raster.h, and to the nine consequences the header states.  No GPU."""
import numpy as np
import pytest

import layer_lcd_ref as ll
import layer_paint_ref as lp
import layer_ref as lr

WEIGHTS = [None, ll.IDENTITY, (0, 16, 64, 176, 0)]


def m(x, y):
    return (x * y + 127) // 255


def brute(plane, image, blits, weights, flags):
    """the header, pixel by pixel"""
    D, E = (t.tolist() for t in lr.srgb_tables())
    W = ll.DEFAULT if weights is None else weights
    rows, stride = image.shape[:2]
    out = image.copy()
    for sx, sy, w, h, dx, dy, rgba in blits:
        def c(q, v):
            return int(plane[sy + v, sx + q]) if 0 <= q < 3 * w and 0 <= v < h else 0
        for v in range(h):
            for u in range(w):
                X, Y = dx + u, dy + v
                if not (0 <= X < stride and 0 <= Y < rows):
                    continue
                f = [(sum(W[i] * c(3 * u + j + i - 2, v) for i in range(5)) + 128) // 256 for j in range(3)]
                if flags & ll.BGR:
                    f = f[::-1]
                a = [m(f[b], rgba[3]) for b in range(3)]
                d = [int(t) for t in image[Y, X]]
                px = []
                for b in range(3):
                    if flags & ll.SRGB:
                        px.append(E[min(65535, (D[rgba[b]] * a[b] + 127) // 255 + (D[d[b]] * (255 - a[b]) + 127) // 255)])
                    else:
                        px.append(min(255, m(rgba[b], a[b]) + m(d[b], 255 - a[b])))
                amax = max(a)
                px.append(amax + m(d[3], 255 - amax))
                out[Y, X] = px
    return out


def _plane(rng, rows, stride):
    """text-like: runs of 0 and 255 with ramps between"""
    p = rng.integers(0, 256, (rows, stride))
    kind = rng.integers(0, 3, (rows, stride))
    return np.where(kind == 0, 0, np.where(kind == 1, 255, p)).astype(np.uint8)


def _image(rng, rows, stride):
    a = rng.integers(0, 256, (rows, stride, 1))
    return np.concatenate([rng.integers(0, 256, (rows, stride, 3)) * a // 255, a], -1).astype(np.uint8)


@pytest.mark.parametrize("flags", [0, 1, 2, 3])
@pytest.mark.parametrize("wi", [0, 1, 2])
def test_twin_equals_the_brute_force(flags, wi):
    """7 x 3 pixel windows at every src_x mod 4, with neighbours in the plane on all sides, whole and clipped"""
    rng = np.random.default_rng(100 * flags + wi)
    for sx in range(4):
        plane, image = _plane(rng, 6, 32), _image(rng, 5, 9)
        colour = tuple(int(v) for v in rng.integers(0, 256, 4))
        for dx, dy in ((1, 1), (-2, -1), (5, 3)):
            blits = [(sx + 1, 2, 7, 3, dx, dy, colour)]
            assert np.array_equal(ll.lcd(plane, image, blits, WEIGHTS[wi], flags), brute(plane, image, blits, WEIGHTS[wi], flags)), (sx, dx, dy)
    # two blits of different colours in one call
    plane, image = _plane(rng, 6, 50), _image(rng, 7, 16)
    blits = [(0, 0, 7, 3, 0, 0, (255, 0, 0, 255)), (23, 3, 7, 3, 8, 2, (0, 200, 90, 130))]
    assert np.array_equal(ll.lcd(plane, image, blits, WEIGHTS[wi], flags), brute(plane, image, blits, WEIGHTS[wi], flags))


def test_srgb_round_trip_is_the_identity():
    """what consequence 1 rests on in linear light: E(D[v]) = v"""
    D, E = lr.srgb_tables()
    assert np.array_equal(E[D], np.arange(256))


@pytest.mark.parametrize("flags", [0, 1, 2, 3])
def test_consequences_1_and_2(flags):
    rng = np.random.default_rng(7)
    plane, image = _plane(rng, 3, 21), _image(rng, 3, 7)
    plane[:, 6:15] = 0
    image[1, :, 3] = 255
    out = ll.lcd(plane, image, [(0, 0, 7, 3, 0, 0, (10, 200, 90, 255))], ll.IDENTITY, flags)
    assert np.array_equal(out[:, 2:5], image[:, 2:5])               # 1: a = (0, 0, 0) leaves the bytes
    assert not np.array_equal(out, image)
    assert (out[1, :, 3] == 255).all()                              # 2: d_a = 255 stays
    out = ll.lcd(plane, image, [(0, 0, 7, 3, 0, 0, (10, 200, 90, 0))], None, flags)
    assert np.array_equal(out, image)                               # A = 0: every a_b is 0


@pytest.mark.parametrize("wi", [0, 1, 2])
def test_consequence_3_white_on_black_shows_f(wi):
    rng = np.random.default_rng(8)
    plane = _plane(rng, 3, 21)
    image = np.zeros((3, 7, 4), np.uint8)
    image[..., 3] = 255
    bl = (0, 0, 7, 3, 0, 0, (255, 255, 255, 255))
    out = ll.lcd(plane, image, [bl], WEIGHTS[wi], 0)
    assert np.array_equal(out[..., :3], ll.filtered(plane, bl, WEIGHTS[wi])) and (out[..., 3] == 255).all()


@pytest.mark.parametrize("wi", [0, 1, 2])
def test_consequences_4_and_9(wi):
    W = ll.DEFAULT if WEIGHTS[wi] is None else WEIGHTS[wi]
    for v in range(256):                                            # 4: a constant run filters to itself (two elements inside the window, beyond which c is 0)
        plane = np.full((1, 29), v, np.uint8)
        assert (ll.filtered(plane, (4, 0, 7, 1), WEIGHTS[wi]).reshape(-1)[2:-2] == v).all()
        assert (256 * v + 128) // 256 == v
    for pos in range(2, 19):                                        # 9: an impulse shows the filter, mirrored
        plane = np.zeros((1, 21), np.uint8)
        plane[0, pos] = 255
        f = ll.filtered(plane, (0, 0, 7, 1), WEIGHTS[wi]).reshape(-1)
        want = np.zeros(21, np.int64)
        want[pos - 2:pos + 3] = [(255 * W[4 - k] + 128) // 256 for k in range(5)]
        assert np.array_equal(f, want), pos


@pytest.mark.parametrize("flags", [0, 1, 2, 3])
def test_consequence_5_identity_filter_is_a_one_stop_paint(flags):
    rng = np.random.default_rng(9)
    k = _plane(rng, 4, 9)
    plane = np.repeat(k, 3, axis=1)
    image = _image(rng, 6, 11)
    layer = np.zeros((4, 9, 4), np.uint8)
    layer[..., 3] = k
    colour = (200, 30, 90, 180)
    for dx, dy in ((1, 1), (-3, -2), (6, 4)):
        got = ll.lcd(plane, image, [(0, 0, 9, 4, dx, dy, colour)], ll.IDENTITY, flags)
        want = lp.paint(image, layer, (0, 0, 9, 4), (dx, dy), (lp.LINEAR, lp.PAD, (0, 0, 640, 0), [(0, colour)]), srgb=bool(flags & 1))
        assert np.array_equal(got, want), (dx, dy)


def test_consequence_6_premultiplied_stays_premultiplied():
    rng = np.random.default_rng(10)
    plane, image = _plane(rng, 16, 96), _image(rng, 16, 32)
    assert (image[..., :3] <= image[..., 3:]).all()
    for colour in ((255, 255, 255, 255), (255, 0, 128, 200), (3, 250, 9, 77)):
        out = ll.lcd(plane, image, [(0, 0, 32, 16, 0, 0, colour)], None, 0)
        assert (out[..., :3] <= out[..., 3:]).all()
    a = np.arange(256)
    for d_a in range(256):                                          # g(a) = a + m(d_a, 255 - a) does not decrease
        g = a + lr.m(d_a, 255 - a)
        assert (np.diff(g) >= 0).all() and g.max() <= 255


@pytest.mark.parametrize("flags", [0, 3])
def test_consequence_7_src_x_moves_the_image(flags):
    rng = np.random.default_rng(11)
    plane = _plane(rng, 3, 40)
    image = np.zeros((3, 9, 4), np.uint8)
    image[..., 3] = 255
    colour = (255, 255, 255, 255)
    at = lambda sx, w: ll.lcd(plane, image, [(sx, 0, w, 3, 0, 0, colour)], ll.IDENTITY, flags)
    # by one pixel: the window's inner pixels agree (the outer ones see other zeros beyond the window only with a wider filter)
    assert np.array_equal(at(3, 8)[:, 1:8], at(6, 7)[:, 0:7])
    # by one sub-pixel: the filtered sub-pixels, read as one row, move by one (away from the window's ends, whose taps differ)
    for w in WEIGHTS:
        f0, f1 = ll.filtered(plane, (3, 0, 9, 3), w).reshape(3, -1), ll.filtered(plane, (4, 0, 8, 3), w).reshape(3, -1)
        assert np.array_equal(f1[:, 2:20], f0[:, 3:21])


@pytest.mark.parametrize("srgb", [0, 1])
@pytest.mark.parametrize("wi", [0, 2])
def test_consequence_8_bgr_is_a_byte_swap(srgb, wi):
    rng = np.random.default_rng(12)
    plane, image = _plane(rng, 5, 40), _image(rng, 5, 12)
    colour = (200, 30, 90, 180)
    swap = lambda im: im[..., [2, 1, 0, 3]]
    got = ll.lcd(plane, image, [(2, 0, 12, 5, 0, 0, colour)], WEIGHTS[wi], srgb | ll.BGR)
    want = swap(ll.lcd(plane, swap(image), [(2, 0, 12, 5, 0, 0, (90, 30, 200, 180))], WEIGHTS[wi], srgb))
    assert np.array_equal(got, want)

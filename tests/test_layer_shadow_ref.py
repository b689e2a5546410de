"""The numpy twin of fr_layer_shadow (tests/layer_shadow_ref.py) held to a brute-force loop over the header's definition,
to the header's six consequences, and the reciprocal constants of the box division (csrc/fr_layer_shadow_plan.cpp, printed
by host/layer_shadow_selftest) to every numerator they can meet.  No GPU."""
import numpy as np
import pytest

import host_selftest
import layer_ref as lr
import layer_shadow_ref as sr


def _brute(a0, s, r, p):
    """A_last on the window grown by R, pixel by pixel from the definition"""
    h, w = a0.shape
    R = sr.reach(s, r, p)
    P = R + 3                                                   # the canvas: beyond R + the largest radius nothing is non-zero
    cur = np.zeros((h + 2 * P, w + 2 * P), np.int64)
    cur[P:P + h, P:P + w] = a0
    stages = ([("max", s)] if s else []) + ([("box", r)] * p if r and p else [])
    for kind, k in stages:
        nxt = np.zeros_like(cur)
        for y in range(k, cur.shape[0] - k):
            for x in range(k, cur.shape[1] - k):
                nb = cur[y - k:y + k + 1, x - k:x + k + 1]
                W = (2 * k + 1) ** 2
                nxt[y, x] = nb.max() if kind == "max" else (int(nb.sum()) + W // 2) // W
        cur = nxt
    return cur[P - R:P + h + R, P - R:P + w + R]


@pytest.mark.parametrize("shape", [(7, 9), (1, 1), (3, 8), (5, 2)], ids=lambda s: "%dx%d" % (s[1], s[0]))
def test_twin_is_the_definition(shape):
    rng = np.random.default_rng(shape[0] * 16 + shape[1])
    a0 = rng.integers(0, 256, shape)
    a0[rng.integers(0, 3, shape) == 0] = 255
    a0[rng.integers(0, 3, shape) == 0] = 0
    for s in range(3):
        for r in range(4):
            for p in range(4):
                got = sr.alpha_plane(a0, s, r, p)
                assert np.array_equal(got, _brute(a0, s, r, p)), (s, r, p)


@pytest.fixture(scope="module")
def layer():
    rng = np.random.default_rng(21)
    a = rng.integers(0, 256, (11, 13, 1))
    a[rng.integers(0, 3, (11, 13, 1)) == 0] = 0
    return np.concatenate([rng.integers(0, 256, (11, 13, 3)) * a // 255, a], -1).astype(np.uint8)


def test_consequence_1_identity(layer):
    got = sr.shadow_rect(layer, (0, 0, 13, 11), (13, 11), (0, 0), 0, 0, 0, (255, 255, 255, 255))
    assert np.array_equal(got, np.repeat(layer[..., 3:], 4, -1))
    for r, p in ((5, 0), (0, 3)):
        assert np.array_equal(sr.shadow_rect(layer, (0, 0, 13, 11), (13, 11), (0, 0), 0, r, p, (255, 255, 255, 255)), got)


def test_consequence_2_constant_neighbourhoods():
    for v in (0, 1, 77, 254, 255):
        a0 = np.full((30, 30), v)
        for s, r, p in ((0, 3, 1), (2, 3, 2), (1, 2, 3), (0, 7, 2)):
            R = sr.reach(s, r, p)
            inner = sr.alpha_plane(a0, s, r, p)[2 * R:30, 2 * R:30]
            assert inner.size and (inner == v).all(), (v, s, r, p)
    for r in range(1, 33):
        W = (2 * r + 1) ** 2
        assert all((v * W + W // 2) // W == v for v in range(256))


def test_consequence_3_reach(layer):
    for s, r, p in ((0, 0, 0), (2, 0, 0), (0, 3, 2), (1, 2, 3)):
        R = sr.reach(s, r, p)
        one = np.zeros((9, 9, 4), np.uint8)
        one[4, 4, 3] = 200
        got = sr.shadow_rect(one, (0, 0, 9, 9), (9 + 2 * R + 4, 9 + 2 * R + 4), (R + 2, R + 2), s, r, p, (9, 9, 9, 255))[..., 3]
        ys, xs = np.nonzero(got)
        c = 4 + R + 2
        assert ys.size and max(abs(ys - c).max(), abs(xs - c).max()) <= R, (s, r, p)
        # a rectangle padded by R holds everything: the sum of alpha over a larger one is the same
        pad = sr.shadow_rect(layer, (0, 0, 13, 11), (13 + 2 * R, 11 + 2 * R), (R, R), s, r, p, (0, 0, 0, 255))[..., 3].astype(np.int64)
        more = sr.shadow_rect(layer, (0, 0, 13, 11), (13 + 2 * R + 6, 11 + 2 * R + 6), (R + 3, R + 3), s, r, p, (0, 0, 0, 255))[..., 3].astype(np.int64)
        assert pad.sum() == more.sum() and np.array_equal(more[3:-3, 3:-3], pad)
        # out of reach: all zero, whichever side
        for off in ((20 + R, 0), (-(13 + R), 0), (0, 20 + R), (0, -(11 + R)), (2 ** 31 - 1, -2 ** 31)):
            assert not sr.shadow_rect(layer, (0, 0, 13, 11), (20, 20), off, s, r, p, (255, 255, 255, 255)).any(), (s, r, p, off)


def test_consequence_4_translation(layer):
    base = sr.shadow_rect(layer, (0, 0, 13, 11), (40, 40), (10, 10), 1, 2, 2, (10, 200, 30, 180))
    for dx, dy in ((1, 0), (0, 1), (-1, 0), (3, -2)):
        got = sr.shadow_rect(layer, (0, 0, 13, 11), (40, 40), (10 + dx, 10 + dy), 1, 2, 2, (10, 200, 30, 180))
        assert np.array_equal(got, np.roll(base, (dy, dx), (0, 1)))


def test_consequence_5_transpose(layer):
    t = np.ascontiguousarray(layer.transpose(1, 0, 2))
    for srgb in (False, True):
        a = sr.shadow_rect(layer, (1, 2, 11, 8), (30, 25), (4, 7), 2, 3, 2, (10, 200, 30, 180), srgb)
        b = sr.shadow_rect(t, (2, 1, 8, 11), (25, 30), (7, 4), 2, 3, 2, (10, 200, 30, 180), srgb)
        assert np.array_equal(a.transpose(1, 0, 2), b)


def test_consequence_6_impulse():
    one = np.zeros((1, 1, 4), np.uint8)
    one[0, 0, 3] = 255
    for r in (1, 2, 3, 7, 16, 32):
        W = (2 * r + 1) ** 2
        got = sr.shadow_rect(one, (0, 0, 1, 1), (2 * r + 5, 2 * r + 5), (r + 2, r + 2), 0, r, 1, (255, 255, 255, 255))[..., 3]
        want = np.zeros_like(got)
        want[2:-2, 2:-2] = (255 + W // 2) // W
        assert np.array_equal(got, want), r


def test_window_cuts_off_the_layer_outside(layer):
    """alpha just outside the window does not leak in"""
    cut = np.zeros_like(layer)
    cut[3:8, 2:9] = layer[3:8, 2:9]
    a = sr.shadow_rect(layer, (2, 3, 7, 5), (20, 20), (6, 6), 1, 2, 2, (1, 2, 3, 255))
    b = sr.shadow_rect(cut, (0, 0, 13, 11), (20, 20), (6 - 2, 6 - 3), 1, 2, 2, (1, 2, 3, 255))
    assert np.array_equal(a, b) and a.any()


def test_tint_is_the_text_plans_sample():
    """the UNORM and sRGB forms of the header, value by value, for every (alpha, A) and a sweep of colours"""
    D, E = lr.srgb_tables()
    al, A = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    a = (al * A + 127) // 255
    for C in (0, 1, 127, 128, 254, 255):
        got = np.stack([sr.tint(al[:, k], (C, 255 - C, C, k), False) for k in range(256)], 1)
        assert np.array_equal(got[..., 0], (C * a + 127) // 255) and np.array_equal(got[..., 3], a)
        got = np.stack([sr.tint(al[:, k], (C, 255 - C, C, k), True) for k in range(256)], 1)
        assert np.array_equal(got[..., 1], E[(D[255 - C] * a + 127) // 255]) and np.array_equal(got[..., 3], a)


def test_reciprocal_constants_are_exact():
    """the kernel divides by W = (2 r + 1)^2 as (n * m) >> (32 + shift) with the constants shadow_recip() hands it: every
    numerator 0 .. 255 W + W div 2 of every radius 1 .. 32"""
    seen = {}
    for line in host_selftest.lines("layer_shadow_selftest"):
        if line.startswith("recip/"):
            name, m, shift = line.split(" ")
            seen[int(name.split("/")[1])] = (int(m.split("=")[1]), int(shift.split("=")[1]))
    assert sorted(seen) == list(range(1, 33))
    for r, (m, shift) in seen.items():
        W = (2 * r + 1) ** 2
        assert 0 < m < 2 ** 32 and 2 ** shift <= W < 2 ** (shift + 1)
        n = np.arange(255 * W + W // 2 + 1, dtype=np.uint64)
        assert n[-1] < 2 ** 21
        got = ((n * np.uint64(m)) >> np.uint64(32)) >> np.uint64(shift)            # v_mul_hi_u32, then the shift
        assert np.array_equal(got, n // np.uint64(W)), r

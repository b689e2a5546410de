"""The numpy twin of fr_layer_mask (tests/layer_mask_ref.py) on the CPU: against a per-pixel brute force in Python ints
written from the header's definition, every (k, o) -> t, and the header's consequences 1 - 7, the ones that name another call
against that call's twin.  No GPU."""
import itertools

import numpy as np
import pytest

import layer_mask_ref as mr
import layer_paint_ref as pr
import layer_rects_ref as rr
import layer_ref as lr
from layer_gpu import premultiplied

SPACES = pytest.mark.parametrize("srgb", [False, True], ids=["unorm", "srgb"])


def _m(x, y):
    return (x * y + 127) // 255


def _brute(layer, mask, image, blits, srgb, erase):
    """the header's definition pixel by pixel, Python ints only"""
    D, E = (t.tolist() for t in lr.srgb_tables())
    out = image.copy()
    rows, stride = image.shape[:2]
    for sx, sy, w, h, dx, dy, mx, my, o, inv in blits:
        for v in range(h):
            for u in range(w):
                X, Y = dx + u, dy + v
                if not (0 <= X < stride and 0 <= Y < rows):
                    continue
                k = int(mask[my + v, mx + u, 3] if mask.ndim == 3 else mask[my + v, mx + u])
                t = _m(255 - k if inv else k, o)
                d = [int(x) for x in image[Y, X]]
                if erase:
                    px = [E[(D[d[c]] * (255 - t) + 127) // 255] if srgb else _m(d[c], 255 - t) for c in range(3)] + [_m(d[3], 255 - t)]
                else:
                    s = [int(x) for x in layer[sy + v, sx + u]]
                    a1 = _m(s[3], t)
                    if srgb:
                        px = [E[min(65535, (D[s[c]] * t + 127) // 255 + (D[d[c]] * (255 - a1) + 127) // 255)] for c in range(3)]
                    else:
                        px = [min(255, _m(s[c], t) + _m(d[c], 255 - a1)) for c in range(3)]
                    px.append(a1 + _m(d[3], 255 - a1))
                out[Y, X] = px
    return out


@pytest.fixture(scope="module")
def small():
    rng = np.random.default_rng(21)
    layer, image = premultiplied(rng, (9, 13)), premultiplied(rng, (10, 11))
    layer[0, :3] = (255, 200, 255, 100)                         # not premultiplied: the clamp
    mask = premultiplied(rng, (12, 15))
    plane = rng.integers(0, 256, (12, 15)).astype(np.uint8)
    plane[0, :4] = (0, 1, 254, 255)
    return layer, mask, plane, image


BLITS = [(1, 2, 7, 5, -2, -1, 3, 4, 255, 0), (0, 0, 4, 3, 6, 0, 11, 9, 128, 1), (5, 5, 6, 4, 5, 6, 0, 0, 1, 0), (0, 0, 3, 3, 0, 7, 2, 2, 0, 1),
         (0, 0, 0, 5, 0, 0, 0, 0, 255, 0), (2, 2, 2, 2, 100, 100, 0, 0, 255, 1)]


@SPACES
@pytest.mark.parametrize("erase", [False, True], ids=["composite", "erase"])
@pytest.mark.parametrize("plane", [False, True], ids=["layer_mask", "plane"])
@pytest.mark.parametrize("flip", [False, True], ids=["as_listed", "inverts_flipped"])
def test_the_twin_is_the_brute_force(small, srgb, erase, plane, flip):
    layer, mask, pl, image = small
    blits = [b[:9] + (b[9] ^ int(flip),) for b in BLITS]
    k = pl if plane else mask
    got = mr.composite(None if erase else layer, k, image, blits, srgb, erase)
    assert np.array_equal(got, _brute(layer, k, image, blits, srgb, erase))
    assert not np.array_equal(got, image)


def test_every_k_and_o():
    k, o = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    for inv in (False, True):
        got = mr.t_of(k, o, inv)
        want = np.array([[_m(255 - a if inv else a, b) for b in range(256)] for a in range(256)])
        assert np.array_equal(got, want)
    t = mr.t_of(k, o)
    assert np.array_equal(t[255], np.arange(256)) and np.array_equal(t[:, 255], np.arange(256)) and not t[0].any() and not t[:, 0].any()
    assert np.array_equal(t, t.T) and t.max() == 255


@pytest.fixture(scope="module")
def scene():
    rng = np.random.default_rng(22)
    return premultiplied(rng, (20, 30)), premultiplied(rng, (25, 40))


@SPACES
def test_consequence_1_a_full_mask_is_fr_layer_over(scene, srgb):
    layer, image = scene
    rows = [(2, 1, 20, 15, -3, 4, 255), (0, 0, 10, 5, 25, 0, 77), (0, 16, 30, 4, 5, 20, 0)]
    want = lr.composite(layer, image, rows, srgb)
    for value, inv in ((255, 0), (0, 1)):
        blits = [r[:6] + (r[0], r[1], r[6], inv) for r in rows]
        assert np.array_equal(mr.composite(layer, np.full((20, 30), value, np.uint8), image, blits, srgb), want)
        full = np.zeros((20, 30, 4), np.uint8)
        full[..., 3] = value
        assert np.array_equal(mr.composite(layer, full, image, blits, srgb), want)


@SPACES
@pytest.mark.parametrize("erase", [False, True], ids=["composite", "erase"])
def test_consequence_2_t_0_leaves_the_pixel(srgb, erase):
    """every destination byte value in every channel, under every layer pixel of the fixture"""
    v = np.arange(256, dtype=np.uint8)
    image = np.stack([v, v[::-1], np.roll(v, 50), v], -1)[None].repeat(4, 0)
    layer = premultiplied(np.random.default_rng(2), (4, 256))
    for plane_value, o, inv in ((0, 255, 0), (255, 255, 1), (200, 0, 0), (1, 127, 0), (254, 127, 1)):
        assert mr.t_of(plane_value, o, inv) == 0
        got = mr.composite(None if erase else layer, np.full((4, 256), plane_value, np.uint8), image, [(0, 0, 256, 4, 0, 0, 0, 0, o, inv)], srgb, erase)
        assert np.array_equal(got, image)


def test_consequence_3_a_premultiplied_layer_never_reaches_the_clamp():
    """m(s_c, t) <= m(s_a, t) for s_c <= s_a, so m(s_c, t) + m(d_c, 255 - a') <= a' + (255 - a') for every t"""
    t = np.arange(256)[:, None, None]
    a = np.arange(256)[None, :, None]
    c = np.arange(256)[None, None, :]
    ok = c <= a
    assert (lr.m(c, t) <= lr.m(a, t))[np.broadcast_to(ok, (256, 256, 256))].all()
    assert (lr.m(a, t) + lr.m(255, 255 - lr.m(a, t)) == 255).all()


@SPACES
def test_consequence_4_a_solid_layer_is_fr_layer_paint(scene, srgb):
    mask, image = scene
    for colour, o in (((200, 10, 99), 255), ((255, 255, 255), 128), ((0, 7, 250), 1)):
        solid = np.zeros((20, 30, 4), np.uint8)
        solid[:] = colour + (255,)
        got = mr.composite(solid, mask, image, [(3, 2, 25, 17, -4, 6, 3, 2, o, 0)], srgb)
        grad = (pr.LINEAR, 0, (0, 0, 64, 0), [(0, colour + (o,))])
        assert np.array_equal(got, pr.paint(image, mask, (3, 2, 25, 17), (-4, 6), grad, srgb))
        assert not np.array_equal(got, image)


@SPACES
@pytest.mark.parametrize("erase", [False, True], ids=["composite", "erase"])
def test_consequence_5_a_plane_is_a_layer_masks_alpha(scene, srgb, erase):
    layer, image = scene
    mask = premultiplied(np.random.default_rng(5), (22, 33))
    blits = [(1, 1, 20, 15, 2, 3, 5, 6, 200, 0), (0, 0, 8, 4, 30, 20, 0, 0, 255, 1)]
    want = mr.composite(None if erase else layer, mask, image, blits, srgb, erase)
    assert np.array_equal(mr.composite(None if erase else layer, np.ascontiguousarray(mask[..., 3]), image, blits, srgb, erase), want)


@SPACES
def test_consequence_6_erase(scene, srgb):
    _, image = scene
    plane = np.random.default_rng(6).integers(0, 256, (25, 40)).astype(np.uint8)
    plane[:5, :8] = 255
    got = mr.composite(None, plane, image, [(0, 0, 40, 25, 0, 0, 0, 0, 255, 0)], srgb, True)
    assert not got[:5, :8].any()                                # t = 255 stores (0, 0, 0, 0)
    for o in (255, 200, 1):
        got = mr.composite(None, plane, image, [(0, 0, 40, 25, 0, 0, 0, 0, o, 0)], srgb, True)
        assert (got[..., 3] <= image[..., 3]).all()             # a destination alpha never grows
    # every (d_a, t): never grows
    d, t = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    assert (lr.m(d, 255 - t) <= d).all()
    for o in (255, 128, 3, 0):
        got = mr.composite(None, np.full((25, 40), 255, np.uint8), image, [(0, 0, 30, 20, 4, 2, 3, 1, o, 0)], srgb, True)
        want = rr.rects(image, [(64 * 4, 64 * 2, 64 * 34, 64 * 22, (0, 0, 0, o))], srgb)
        assert np.array_equal(got[..., :3], want[..., :3])
        if 0 < o:                                               # the alpha differs by definition: o + m(d_a, 255 - o) against m(d_a, 255 - o)
            inside = (slice(2, 22), slice(4, 34))
            assert np.array_equal(want[inside][..., 3].astype(int) - got[inside][..., 3], np.full((20, 30), o))


@SPACES
@pytest.mark.parametrize("erase", [False, True], ids=["composite", "erase"])
def test_consequence_7_invert_is_the_complemented_mask(scene, srgb, erase):
    layer, image = scene
    mask = premultiplied(np.random.default_rng(7), (22, 33))
    for o, plane in itertools.product((255, 100), (False, True)):
        k = np.ascontiguousarray(mask[..., 3]) if plane else mask
        comp = 255 - k if plane else np.concatenate([mask[..., :3], 255 - mask[..., 3:]], -1)
        a = mr.composite(None if erase else layer, k, image, [(0, 0, 20, 15, 2, 3, 5, 6, o, 1)], srgb, erase)
        b = mr.composite(None if erase else layer, comp, image, [(0, 0, 20, 15, 2, 3, 5, 6, o, 0)], srgb, erase)
        assert np.array_equal(a, b)

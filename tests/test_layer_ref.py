"""The twin of fr_layer_over (tests/layer_ref.py) on the CPU: m against round-to-nearest in exact fractions for every
(x, y), the alpha bound for every (s_a, d_a, o), and the header's consequences 1 to 4 over their whole domains.  The twin's
unpremultiply is held to the library's host function fr_rgba_unpremultiply on every (c, a), and the reciprocal table of
the device kernel (csrc/fr_layer.hip: M = ceil(2^36 / a)) to integer division over its whole domain."""
from fractions import Fraction

import numpy as np

import font_renderer_amd as fr
import layer_ref as lr

V = np.arange(256, dtype=np.int64)


def test_m_is_round_to_nearest_in_exact_fractions():
    got = lr.m(V[:, None], V[None, :])
    for x in range(256):
        for y in range(256):
            q = Fraction(x * y, 255)
            n = int(got[x, y])
            assert abs(q - n) < Fraction(1, 2), (x, y, n)          # strictly: 255 is odd, no ties
    assert np.array_equal(lr.m(V, 255), V) and not lr.m(V, 0).any() and not lr.m(0, V).any()


def test_srgb_tables_round_trip():
    D, E = lr.srgb_tables()
    assert np.array_equal(E[D], V) and D[0] == 0 and D[255] == 65535


def test_alpha_never_exceeds_255_and_an_opaque_destination_stays_opaque():
    s_a, d_a, o = np.meshgrid(V, V, V, indexing="ij")
    out = lr.over_alpha(s_a, d_a, o)
    assert out.min() >= 0 and out.max() <= 255                      # the bound, every (s_a, d_a, o)
    assert (out[:, 255, :] == 255).all()                            # consequence 3, every (s_a, o)
    assert np.array_equal(out[0], np.broadcast_to(V[:, None], (256, 256)))      # s_a = 0: d_a for every o


def test_consequence_1_a_zero_pixel_or_zero_opacity_changes_nothing():
    for srgb in (False, True):
        # s = (0, 0, 0, 0): every (o, d_c)
        o, d = np.meshgrid(V, V, indexing="ij")
        assert np.array_equal(lr.over_colour(0, 0, d, o, srgb), d)
        # o = 0: every (s_c, s_a, d_c), valid premultiplied or not
        s_c, s_a, d_c = np.meshgrid(V, V, V, indexing="ij")
        assert np.array_equal(lr.over_colour(s_c, s_a, d_c, 0, srgb), d_c)
    assert np.array_equal(lr.over_alpha(V[:, None], V[None, :], 0), np.broadcast_to(V[None, :], (256, 256)))


def test_consequence_2_an_opaque_pixel_at_full_opacity_replaces():
    s_c, d_c = np.meshgrid(V, V, indexing="ij")
    for srgb in (False, True):
        assert np.array_equal(lr.over_colour(s_c, 255, d_c, 255, srgb), s_c)
    assert (lr.over_alpha(255, V, 255) == 255).all()


def test_consequence_4_a_premultiplied_unorm_pixel_never_reaches_the_clamp():
    """m(d, ia) does not fall as d grows (every (d, ia)), so the largest sum is at d_c = 255; there, for every
    (s_c <= s_a, o), m(s_c, o) + m(255, 255 - a') <= 255"""
    md = lr.m(V[:, None], V[None, :])
    assert (np.diff(md, axis=0) >= 0).all()
    s_c, s_a, o = np.meshgrid(V, V, V, indexing="ij")
    raw = lr.over_colour_raw(s_c, s_a, 255, o)
    assert raw[s_c <= s_a].max() == 255
    assert raw.max() > 255                                          # without s_c <= s_a the clamp is reached: it is needed


def test_unpremultiply_twin_is_the_host_function():
    c, a = np.meshgrid(V, V, indexing="ij")
    for srgb in (False, True):
        px = np.stack([c, 255 - c, (c * 7 + a) % 256, a], -1).astype(np.uint8).reshape(-1, 4)
        im = fr.RGBA(256, 256, px.copy()).unpremultiply(srgb)
        assert np.array_equal(im.data, lr.unpremultiply(px, srgb))
        opaque = px[px[:, 3] == 255]
        assert np.array_equal(lr.unpremultiply(opaque, srgb), opaque)


def test_reciprocal_table_divides_exactly():
    """(n * ceil(2^36 / a)) >> 36 == n div a for n = 255 x + a div 2, every x in 0 .. 65535 and a in 1 .. 255"""
    x = np.arange(65536, dtype=np.uint64)
    for a in range(1, 256):
        n = 255 * x + np.uint64(a // 2)
        M = np.uint64(((1 << 36) + a - 1) // a)
        assert int(n.max()) * int(M) < 1 << 64
        assert np.array_equal((n * M) >> np.uint64(36), n // np.uint64(a)), a

"""The numpy twin of fr_layer_blend (tests/layer_blend_ref.py) on the CPU: against the W3C compositing formula in exact
fractions, against the header's consequences 1 - 6 on arbitrary bytes, and against the twin of fr_layer_over for consequence
3; then the lines of host/layer_blend_selftest.cpp, which holds the text the kernel compiles to a 64-bit restatement and
whose digests are drawn again here for the twin.  No GPU."""
import itertools
from fractions import Fraction

import numpy as np
import pytest

import host_selftest
import layer_blend_ref as br
import layer_ref as lr

SPACES = pytest.mark.parametrize("srgb", [False, True], ids=["unorm", "srgb"])
QS = pytest.mark.parametrize("Q", [255, 65535])
MODES = pytest.mark.parametrize("mode", range(br.MODES), ids=br.NAMES)
SELFTEST = "layer_blend_selftest"


def _w3c(mode, x, y, p, q, Q):
    """Q times co = cs (1 - ab) + cb (1 - as) + as ab B(Cb, Cs) of the W3C compositing specification, an exact Fraction, for
    a premultiplied source value x under alpha p and a premultiplied backdrop value y under alpha q, all out of Q"""
    cs, cb, a_s, a_b = Fraction(x, Q), Fraction(y, Q), Fraction(p, Q), Fraction(q, Q)
    if mode == br.PLUS:
        return Q * min(Fraction(1), cs + cb)
    Cs = Fraction(x, p) if p else Fraction(0)                  # the straight colours; under a zero alpha the term vanishes
    Cb = Fraction(y, q) if q else Fraction(0)

    def hard_light(Cb, Cs):
        return Cb * 2 * Cs if 2 * Cs <= 1 else Cb + (2 * Cs - 1) - Cb * (2 * Cs - 1)
    B = {br.MULTIPLY: lambda: Cb * Cs, br.SCREEN: lambda: Cb + Cs - Cb * Cs, br.OVERLAY: lambda: hard_light(Cs, Cb),
         br.DARKEN: lambda: min(Cb, Cs), br.LIGHTEN: lambda: max(Cb, Cs), br.HARD_LIGHT: lambda: hard_light(Cb, Cs),
         br.DIFFERENCE: lambda: abs(Cb - Cs), br.EXCLUSION: lambda: Cb + Cs - 2 * Cb * Cs}[mode]()
    return Q * (cs * (1 - a_b) + cb * (1 - a_s) + a_s * a_b * B)


def _valid_cases(Q, seed):
    """(x, y, p, q) with x <= p and y <= q: the corners {0, p/2 - 1, p/2, p/2 + 1, p} x {0, q/2 - 1 .. q} for alphas from the
    ends, the middle and in between, and a seeded random sample"""
    alphas = sorted({0, 1, 2, 3, Q // 3, Q // 2, Q // 2 + 1, Q - 1, Q})
    around = lambda a: sorted({v for v in (0, a // 2 - 1, a // 2, a // 2 + 1, a) if 0 <= v <= a})
    cases = [(x, y, p, q) for p in alphas for q in alphas for x in around(p) for y in around(q)]
    rng = np.random.default_rng(seed)
    for _ in range(1500):
        p, q = (int(v) for v in rng.integers(0, Q + 1, 2))
        cases.append((int(rng.integers(0, p + 1)), int(rng.integers(0, q + 1)), p, q))
    return cases


@QS
@MODES
def test_the_twin_is_the_nearest_integer_to_the_w3c_formula(mode, Q):
    """consequence 1: for valid premultiplied inputs N <= Q^2, the error is below 1/2 and never a tie"""
    cases = _valid_cases(Q, 100 + mode)
    x, y, p, q = (np.array(v, np.int64) for v in zip(*cases))
    got = br.channel(mode, x, y, p, q, Q)
    if mode != br.PLUS:
        assert (br.numerator(mode, x, y, p, q, Q) <= Q * Q).all()
    for c, g in zip(cases, got.tolist()):
        exact = _w3c(mode, *c, Q)
        assert abs(g - exact) < Fraction(1, 2), (c, g, exact)
        assert 0 <= g <= Q


def _any_bytes(n, seed):
    """arbitrary pixels, valid premultiplied or not, with the ends of every byte well represented"""
    rng = np.random.default_rng(seed)
    px = rng.integers(0, 256, (n, 4))
    ends = rng.choice([0, 1, 127, 128, 254, 255], (n, 4))
    return np.where(rng.integers(0, 3, (n, 4)) == 0, ends, px).astype(np.uint8)


@pytest.fixture(scope="module")
def pairs():
    """every pair of the corner pixels built from {0, 1, 127, 128, 255} per byte (625 x 625) and 200 000 random pairs"""
    corner = np.array(list(itertools.product((0, 1, 127, 128, 255), repeat=4)), np.uint8)
    a = np.concatenate([np.repeat(corner, len(corner), 0), _any_bytes(200000, 1)])
    b = np.concatenate([np.tile(corner, (len(corner), 1)), _any_bytes(200000, 2)])
    return a, b


@SPACES
@MODES
def test_consequence_2_an_empty_layer_pixel_or_opacity_0_changes_nothing(pairs, mode, srgb):
    a, b = pairs
    assert np.array_equal(br.blend(np.zeros_like(a), b, 255, mode, srgb), b)
    assert np.array_equal(br.blend(np.zeros_like(a), b, 77, mode, srgb), b)
    assert np.array_equal(br.blend(a, b, 0, mode, srgb), b)


@SPACES
@MODES
@pytest.mark.parametrize("o", [255, 128, 1])
def test_consequence_3_over_a_cleared_pixel_every_mode_is_fr_layer_over(pairs, mode, srgb, o):
    a, _ = pairs
    assert np.array_equal(br.blend(a, np.zeros_like(a), o, mode, srgb), lr.over(a, np.zeros_like(a), o, srgb))


@SPACES
@pytest.mark.parametrize("mode", br.SYMMETRIC, ids=[br.NAMES[m] for m in br.SYMMETRIC])
def test_consequence_4_symmetric_modes(pairs, mode, srgb):
    a, b = pairs
    assert np.array_equal(br.blend(a, b, 255, mode, srgb), br.blend(b, a, 255, mode, srgb))


@SPACES
def test_consequence_5_hard_light_is_overlay_swapped(pairs, srgb):
    a, b = pairs
    hard = br.blend(a, b, 255, br.HARD_LIGHT, srgb)
    assert np.array_equal(hard, br.blend(b, a, 255, br.OVERLAY, srgb))
    assert not np.array_equal(hard, br.blend(a, b, 255, br.OVERLAY, srgb))        # (the two are different modes)


@QS
def test_consequence_6_the_numerator_never_exceeds_3_q_squared(Q):
    """any values in [0, Q]; in linear light some N is above 2^32, so 32 bits do not hold it"""
    ends = np.array(list(itertools.product((0, 1, Q // 2, Q // 2 + 1, Q - 1, Q), repeat=4)), np.int64)
    rng = np.random.default_rng(6)
    v = np.concatenate([ends, rng.integers(0, Q + 1, (200000, 4))])
    top = 0
    for mode in range(br.PLUS):
        n = br.numerator(mode, v[:, 0], v[:, 1], v[:, 2], v[:, 3], Q)
        assert (n >= 0).all() and (n <= 3 * Q * Q).all(), br.NAMES[mode]
        top = max(top, int(n.max()))
    assert top == 3 * Q * Q and (top >= 2 ** 32) == (Q == 65535)       # MULTIPLY at x = y = Q, p = q = 0 reaches the bound


def test_every_unorm_colour_pair_against_python_ints():
    """the UNORM twin at every (s_c, d_c) and four alpha pairs against the header's lines in Python ints"""
    s, d = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    for mode, (p, q) in itertools.product(range(br.PLUS), ((255, 255), (255, 128), (128, 255), (77, 200))):
        got = br.channel(mode, s, d, p, q, 255)
        for x, y in ((0, 0), (255, 255), (200, 3), (3, 200), (77, 200), (128, 64), (39, 101)):
            pos = lambda v: max(v, 0)
            light = pos(p * q - 2 * pos(q - y) * pos(p - x))
            b2 = [x * y, pos(x * q + y * p - x * y), 2 * x * y if 2 * y <= q else light, min(x * q, y * p), max(x * q, y * p),
                  2 * x * y if 2 * x <= p else light, abs(x * q - y * p), pos(x * q + y * p - 2 * x * y)][mode]
            assert got[x, y] == min(255, (x * (255 - q) + y * (255 - p) + b2 + 127) // 255), (mode, p, q, x, y)


def test_composite_clips_as_fr_layer_over_does():
    layer, image = _any_bytes(9 * 13, 4).reshape(9, 13, 4), _any_bytes(10 * 11, 5).reshape(10, 11, 4)
    blits = [(1, 2, 8, 6, -3, -2, 255), (0, 0, 4, 4, 9, 8, 100), (0, 0, 3, 3, 11, 0, 255), (5, 5, 0, 2, 0, 0, 255)]
    got = br.composite(layer, image, blits, br.DIFFERENCE)
    assert np.array_equal(got[0:4, 0:5], br.blend(layer[4:8, 4:9], image[0:4, 0:5], 255, br.DIFFERENCE))
    assert np.array_equal(got[8:10, 9:11], br.blend(layer[0:2, 0:2], image[8:10, 9:11], 100, br.DIFFERENCE))
    rest = np.ones(image.shape[:2], bool)
    rest[0:4, 0:5] = rest[8:10, 9:11] = False
    assert np.array_equal(got[rest], image[rest])


# ---- the host self-test: the text the kernel compiles ------------------------------------------------------------------------
def _fields(text):
    return dict(f.split("=", 1) for f in text.split(" ") if "=" in f)


def test_selftest_divisions():
    lines = host_selftest.named(SELFTEST)
    d255, d65535 = _fields(lines["div255"]), _fields(lines["div65535"])
    assert d255 == {"checked": str(2 ** 24), "bad": "0"}
    assert d65535["bad"] == "0" and int(d65535["top"]) == 3 * 65535 ** 2 + 65535
    # every multiple of 65535 up to `top`, one below and one above each (none below 0), and the spread up to 2^47
    assert int(d65535["checked"]) >= 3 * (int(d65535["top"]) // 65535 + 1) - 1


def _lcg(seed):
    s = seed
    while True:
        s = (s * 6364136223846793005 + 1442695040888963407) % 2 ** 64
        yield s >> 33


@QS
def test_selftest_pixels_and_digests(Q):
    """no difference from the 64-bit restatement on the corners and 2 000 000 random draws per mode, no valid input above
    Q^2, and the digest of 4096 outputs equals the twin's on the same draws"""
    lines = host_selftest.named(SELFTEST)
    for mode in range(br.PLUS):
        f = _fields(lines[f"px/{Q}/{br.NAMES[mode]}"])
        assert f["bad"] == "0" and f["valid_over"] == "0" and int(f["corners"]) >= 6 ** 4 and int(f["random"]) == 2000000
        g = _lcg(12345 + mode)
        v = np.array([next(g) % (Q + 1) for _ in range(4 * 4096)], np.int64).reshape(4096, 4)
        digest = 0
        for out in br.channel(mode, v[:, 0], v[:, 1], v[:, 2], v[:, 3], Q).tolist():
            digest = (digest * 31 + out) % 2 ** 64
        assert digest == int(f["digest"]), br.NAMES[mode]


def test_selftest_check_order():
    """the mode check stands straight after the flag bits and before everything fr_layer_over checks"""
    c = {k: v for k, v in host_selftest.named(SELFTEST).items() if k.startswith("check/")}
    assert c["check/valid_plus"] == "rc=0 | tiles=1" and c["check/valid_srgb_multiply"] == "rc=0 | tiles=1"
    assert c["check/mode_9"].startswith("rc=-1 | err=blend mode 9") and c["check/mode_max"].startswith("rc=-1 | err=blend mode 4294967295")
    for k in ("check/flag_before_mode", "check/flag_mask_plane", "check/flag_mask_erase"):
        assert c[k].startswith("rc=-1 | err=unknown flag bits"), k
    for k in ("check/mode_before_src", "check/mode_before_opacity"):
        assert c[k].startswith("rc=-1 | err=blend mode 9"), k
    assert c["check/src_null"] == "rc=-1 | err=src is NULL" and "opacity 256" in c["check/opacity_256"]

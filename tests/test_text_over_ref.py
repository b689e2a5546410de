"""FR_TEXT_OVER on the CPU (include/fr_raster.h): the flag's value in the header and its mirrors, the alpha formula against
rationals, the consequences the header states on the assembled twin (tests/text_twin.py), the exact cases'
own expectations (tests/text_over_cases.py), the blend = 2 lines of host/text_plan_selftest, and fr_rgba_unpremultiply
for every (c, a)."""
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import font_renderer_amd as fr
import host_selftest
import text_block_cases as B
import text_over_cases as OC
import text_twin as tw
from font_renderer_amd import _lib
from fixtures import load_font

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_flag_in_the_mirrors_of_the_header():
    header = open(os.path.join(ROOT, "include", "fr_raster.h")).read()
    assert re.search(r"^#define FR_TEXT_OVER 256u$", header, flags=re.M)
    assert _lib.FR_TEXT_OVER == 256 and fr.FR_TEXT_OVER == 256
    zig = open(os.path.join(ROOT, "bindings", "fr_raster.zig")).read()
    assert re.search(r"^pub const FR_TEXT_OVER: u32 = 256;$", zig, flags=re.M)
    others = _lib.FR_FILL_CONSISTENT | _lib.FR_TEXT_BGRA | _lib.FR_TEXT_SRGB | _lib.FR_TEXT_LOAD | _lib.FR_TEXT_CACHE
    assert others & _lib.FR_TEXT_OVER == 0 and (others | _lib.FR_TEXT_OVER) & (2 | 16 | 64 | 1 << 31) == 0


def test_alpha_formula_is_round_half_up_of_source_over():
    """every (a, A): A/255 + a/255 (1 - A/255), times 255, rounded half up, in rationals; no tie occurs (255 is odd); and
    the twin's R channel under the substitution C = 255 is that value"""
    for A in range(256):
        for a in range(256):
            exact = Fraction(255 * A + a * (255 - A), 255)
            assert (exact * 2).denominator != 2 or exact.denominator == 1
            want = (2 * exact.numerator + exact.denominator) // (2 * exact.denominator)          # floor(exact + 1/2)
            assert tw.alpha_over(a, A) == want, (a, A)
    a, A = np.meshgrid(np.arange(256, dtype=np.int64), np.arange(256, dtype=np.int64), indexing="ij")
    want = tw.alpha_over(a, A)
    assert want.min() == 0 and want.max() == 255 and (want >= np.maximum(a, A) - 0).all()        # over never lowers alpha
    for Ak in (0, 1, 127, 128, 254, 255):
        dst = np.repeat(np.arange(256, dtype=np.int64)[:, None], 4, axis=1)
        assert np.array_equal(tw.blend(dst, (255, 255, 255, Ak))[:, 0], want[:, Ak])
    # what the UNORM kernel computes: x = 255 A + a (255 - A) <= 65025 lies in blend2's proven domain
    assert (255 * A + a * (255 - A)).max() == 65025


@pytest.fixture(scope="module")
def word():
    """one short italic string whose glyphs overlap, as one run with a margin"""
    font = load_font("DejaVuSerif-Italic.ttf")
    gs, places, runs, shape = tw.lines(font, ["fjW"], 17, pad=1)
    places["pen_x64"][:3] = places["pen_x64"][0] + np.array([0, 150, 330])
    return gs, places, runs, shape


COLS = np.array([(200, 30, 90, 160), (20, 220, 140, 77), (250, 250, 10, 201)], np.uint8)
CLEAR = np.array([(10, 60, 90, 128)], np.uint8)


@pytest.mark.parametrize("n,center,fill", [(1, True, False), (2, False, True), (4, True, False)])
@pytest.mark.parametrize("srgb", [False, True])
def test_consequences_on_the_assembled_twin(word, srgb, n, center, fill):
    gs, places, runs, shape = word
    sent = np.full(shape + (4,), 0x5b, np.uint8)
    got = tw.over_render_runs("plain", gs, places, COLS, runs, CLEAR, sent, n, center, fill, srgb)
    plain = tw.rgba_render_runs("plain", gs, places, COLS, runs, CLEAR, sent.copy(), n, center, fill, srgb, False, False)
    assert np.array_equal(got[..., :3], plain[..., :3]) and (got[..., 3] != plain[..., 3]).any()      # 1
    # 2: every A = 255 is the plan without the flag
    opaque = COLS.copy()
    opaque[:, 3] = 255
    assert np.array_equal(tw.over_render_runs("plain", gs, places, opaque, runs, CLEAR, sent, n, center, fill, srgb),
                          tw.rgba_render_runs("plain", gs, places, opaque, runs, CLEAR, sent.copy(), n, center, fill, srgb, False, False))
    # 3: an instance with A = 0 leaves every sample unchanged: the plan without that placement (its glyph has no other)
    zero = COLS.copy()
    zero[1, 3] = 0
    without = np.array(runs).copy()
    two = np.array(places)[[0, 2]]
    without["count"] = 2
    assert np.array_equal(tw.over_render_runs("plain", gs, places, zero, runs, CLEAR, sent, n, center, fill, srgb),
                          tw.over_render_runs("plain", gs, two, zero[[0, 2]], without, CLEAR, sent, n, center, fill, srgb))
    replaced = tw.rgba_render_runs("plain", gs, places, zero, runs, CLEAR, sent.copy(), n, center, fill, srgb, False, False)
    assert (replaced[..., 3] == 0).any() or n > 1                       # (without the flag A = 0 sets alpha to 0)
    # 4: under LOAD over alpha 255 every alpha stays 255
    noise = np.random.default_rng(n).integers(0, 256, shape + (4,)).astype(np.uint8)
    noise[..., 3] = 255
    over = tw.over_render_runs("plain", gs, places, COLS, runs, None, noise, n, center, fill, srgb, False, True)
    assert (over[..., 3] == 255).all() and not np.array_equal(over, noise)
    holes = tw.rgba_render_runs("plain", gs, places, COLS, runs, None, noise.copy(), n, center, fill, srgb, False, True)
    assert (holes[..., 3] != 255).any() and np.array_equal(holes[..., :3], over[..., :3])
    # 5: one instance (R, G, B, A) over (0, 0, 0, 0): alpha = (k A + n^2/2) div n^2 for the k samples it lights
    run1 = np.array(runs).copy()
    run1["count"] = 1
    one = tw.over_render_runs("plain", gs, places, COLS, run1, np.zeros((1, 4), np.uint8), sent, n, center, fill, srgb)
    (_, y0, x0, hit), = tw.instance_hits("plain", gs, places, run1[0], n, center, fill)
    k = np.zeros((int(run1[0]["h"]), int(run1[0]["w"])), np.int64)
    k[y0:y0 + hit.shape[0] // n, x0:x0 + hit.shape[1] // n] = hit.reshape(hit.shape[0] // n, n, hit.shape[1] // n, n).sum(axis=(1, 3))
    oy, ox = int(run1[0]["out_y"]), int(run1[0]["out_x"])
    assert np.array_equal(one[oy:oy + k.shape[0], ox:ox + k.shape[1], 3], (k * int(COLS[0, 3]) + n * n // 2) // (n * n))
    assert k.max() == n * n and (n == 1 or ((k > 0) & (k < n * n)).any())


@pytest.mark.parametrize("form", ["ex", "affine"])
def test_the_other_forms_assemble_alike(word, form):
    """with slant 0 and whole baselines the _ex twin, and with m = {s, 0, 0, s} at a power-of-two size the affine twin, give
    the upright form's image: the assembly goes through each form's own twin"""
    from font_renderer_amd import render_glyph as rg
    gs, places, runs, shape = word
    sent = np.full(shape + (4,), 0x5b, np.uint8)
    ex = rg.make_places_ex([(int(p["glyph"]), int(p["pen_x64"]), 64 * int(p["pen_y"]), 0.0, 0.0) for p in places])
    want = tw.over_render_runs("plain", gs, places, COLS, runs, CLEAR, sent, 2, True, True, True)
    assert np.array_equal(tw.over_render_runs("ex", gs, ex, COLS, runs, CLEAR, sent, 2, True, True, True), want)
    if form == "affine":
        p2 = np.array(runs).copy()
        p2["scale"] = np.float32(2.0 ** -7)
        want = tw.over_render_runs("ex", gs, ex, COLS, p2, CLEAR, sent, 2, True, True, False)
        assert np.array_equal(tw.over_render_runs("affine", gs, tw.from_ex(ex, p2), COLS, p2, CLEAR, sent, 2, True, True, False), want)


@pytest.mark.parametrize("srgb", [False, True])
@pytest.mark.parametrize("n", [2, 4])
def test_partial_cover_case_is_what_it_says(n, srgb):
    """the exact case's geometry through the exact rasteriser of tests/text_block_cases.py: the lit sample counts are
    the k the expectation assumed, the two placement orders differ, and partial coverage occurs"""
    case = OC.partial_cover_case(n, False, srgb)
    nn = n * n
    for r, run in enumerate(case.runs):
        per = {}
        for idx, y0, x0, wd in B.instance_windings(case.glyphs, case.places, run, n, True):
            hit = wd != 0
            k = hit.reshape(hit.shape[0] // n, n, hit.shape[1] // n, n).sum(axis=(1, 3))
            want_k = int(case.places[idx]["glyph"]) + 1
            assert (k[0, :8] == want_k).all() and not k[1:].any() and not k[:, 8:].any(), (r, idx)
            per[idx] = want_k
        assert len(per) == int(run["count"])
    h = nn + 1
    a, b = case.want[1:1 + h, 1:-1], case.want[1 + (h + 1):1 + (h + 1) + h, 1:-1]
    assert (a != b).any() and np.array_equal(a[0], b[0]) and np.array_equal(a[:, :8], b[:, :8])     # orders differ only where both cover
    assert len(np.unique(case.want[..., 3])) > 32


def test_selftest_blend_lines():
    """host/text_plan_selftest over: FR_TEXT_OVER changes no table, and blend is 2 for translucent colours, 0 for opaque"""
    got = host_selftest.named("text_plan_selftest", "over")
    assert len(got) == 36
    field = {k: re.fullmatch(r"([0-9a-f]{16}) insts (\d+) blend ([012])", v).groups() for k, v in got.items()}
    for name, translucent in (("translucent", True), ("opaque", False), ("alpha_zero_srgb_bgra", True), ("load_srgb", True),
                              ("load_opaque", False), ("translucent_clipped_away", True)):
        for form in ("plain", "ex", "affine"):
            plain, over = field[f"{name}/{form}"], field[f"{name}_over/{form}"]
            assert plain[:2] == over[:2], (name, form)
            assert (plain[2], over[2]) == (("1", "2") if translucent else ("0", "0")), (name, form)


def _unpremultiply_want(c, a, srgb):
    if a == 0:
        return 0
    if not srgb:
        return min(255, (255 * c + a // 2) // a)
    return int(tw.E[min(65535, (255 * int(tw.D[c]) + a // 2) // a)])


@pytest.mark.parametrize("srgb", [False, True])
def test_unpremultiply_every_c_a(srgb):
    """fr_rgba_unpremultiply and RGBA.unpremultiply against the header's formula in Python integers, for every (c, a)"""
    c, a = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    px = np.stack([c, (c + 85) % 256, (c * 7 + 3) % 256, a], axis=-1).reshape(-1, 4).astype(np.uint8)
    im = fr.RGBA(256, 256, px.copy())
    assert im.unpremultiply(srgb=srgb) is im
    table = np.array([[_unpremultiply_want(cc, aa, srgb) for aa in range(256)] for cc in range(256)], np.uint8)
    want = px.copy()
    for ch in range(3):
        want[:, ch] = table[px[:, ch], px[:, 3]]
    assert np.array_equal(im.data, want)
    assert np.array_equal(im.data[:, 3], px[:, 3])
    opaque = px[px[:, 3] == 255]
    assert len(opaque) == 256 and np.array_equal(im.data[px[:, 3] == 255], opaque)      # a = 255: unchanged (E(D[v]) = v)
    assert not im.data[px[:, 3] == 0].any()
    lib = fr.load_library()
    assert lib.fr_rgba_unpremultiply(None, 1, 0) == -1 and lib.fr_rgba_unpremultiply(None, 0, 1) == 0

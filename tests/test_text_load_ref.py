"""FR_TEXT_LOAD on the CPU: the flag's value in the header, the Python binding and the Zig binding, and the CPU twin
(tests/text_twin.py) against the consequences the definition states (include/fr_raster.h): untouched pixels come
back byte-identical, and a uniform destination gives the clear-colour plans' twins."""
import os
import re

import numpy as np
import pytest

import font_renderer_amd as fr
import text_twin as tw
from font_renderer_amd import _lib
from fixtures import load_font

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_flag_value_everywhere():
    with open(os.path.join(ROOT, "include", "fr_raster.h")) as f:
        assert re.search(r"^#define FR_TEXT_LOAD 32u$", f.read(), re.M)
    with open(os.path.join(ROOT, "bindings", "fr_raster.zig")) as f:
        assert re.search(r"^pub const FR_TEXT_LOAD: u32 = 32;", f.read(), re.M)
    assert _lib.FR_TEXT_LOAD == fr.FR_TEXT_LOAD == 32
    assert not fr.FR_TEXT_LOAD & (fr.FR_TEXT_SRGB | fr.FR_TEXT_BGRA | fr.FR_FILL_CONSISTENT | 2 | 16)
    assert callable(fr.draw_text_rgba)


def test_decode_then_encode_is_the_identity():
    """consequence 1 for sRGB: E(D[v]) = v for all 256 values"""
    assert np.array_equal(tw.srgb_encode(tw.D), np.arange(256))


@pytest.fixture(scope="module")
def italic():
    font = load_font("DejaVuSerif-Italic.ttf")
    gs, places, runs, shape = tw.lines(font, ["ffi fj Tf", "Wavy /// fff", "WoWfj"], 19, pad=1)
    k0 = int(runs[2]["first"])                                  # glyphs packed so close that their ink overlaps
    places["pen_x64"][k0:k0 + 5] = places["pen_x64"][k0] + np.array([0, 203, 390, 611, 777])
    return gs, places, runs, shape


def _colours(k, seed, opaque):
    c = np.random.default_rng(seed).integers(0, 256, (k, 4)).astype(np.uint8)
    if opaque:
        c[:, 3] = 255
    return c


@pytest.mark.parametrize("srgb", [False, True])
@pytest.mark.parametrize("n,center,fill,opaque", [(1, False, False, True), (2, True, True, False), (4, True, False, False),
                                                  (4, False, True, True)])
def test_uniform_destination_is_the_clear_colour_plan(italic, srgb, n, center, fill, opaque):
    """consequence 2: a destination holding Q_r in every pixel of run r gives the plan without FR_TEXT_LOAD"""
    gs, places, runs, _ = italic
    cols = _colours(len(places), 3 + n, opaque)
    for r, run in enumerate(runs):
        q = tuple(int(v) for v in np.random.default_rng(r).integers(0, 256, 4))
        dst = np.empty((int(run["h"]), int(run["w"]), 4), np.uint8)
        dst[:] = q
        got = tw.rgba_render_run("plain", gs, places, cols, run, None, dst, n, center, fill, srgb)
        assert np.array_equal(got, tw.rgba_render_run("plain", gs, places, cols, run, q, None, n, center, fill, srgb)), (r, srgb, n)
        if srgb:                           # FR_TEXT_BGRA: the same, read and written as B G R A
            got = tw.rgba_render_run("plain", gs, places, cols, run, None, tw.bgra(dst), n, center, fill, srgb, bgr=True)
            assert np.array_equal(got, tw.rgba_render_run("plain", gs, places, cols, run, q, None, n, center, fill, True, bgr=True))


@pytest.mark.parametrize("srgb", [False, True])
@pytest.mark.parametrize("n", [1, 2, 4])
def test_untouched_pixels_are_identical(italic, srgb, n):
    """consequence 1: a pixel at which no instance lights a sample comes back byte for byte, on random destinations"""
    gs, places, runs, _ = italic
    cols = _colours(len(places), n, opaque=False)
    rng = np.random.default_rng(40 + n)
    changed = 0
    for run in runs:
        h, w = int(run["h"]), int(run["w"])
        dst = rng.integers(0, 256, (h, w, 4)).astype(np.uint8)
        lit = np.zeros((h * n, w * n), bool)
        for k, y0, x0, hit in tw.instance_hits("plain", gs, places, run, n, True):
            lit[y0 * n:y0 * n + hit.shape[0], x0 * n:x0 * n + hit.shape[1]] |= hit
        lit = lit.reshape(h, n, w, n).any(axis=(1, 3))
        for bgr in (False, True):
            got = tw.rgba_render_run("plain", gs, places, cols, run, None, dst, n, True, False, srgb, bgr)
            assert np.array_equal(got[~lit], dst[~lit]), (srgb, n, bgr)
            changed += int((got[lit] != dst[lit]).any(axis=1).sum())
    assert changed > 0


def test_second_render_composites_over_the_first(italic):
    """consequence 3: not idempotent for translucent text"""
    gs, places, runs, shape = italic
    cols = _colours(len(places), 9, opaque=False)
    cols[:, 3] = 120
    out = np.random.default_rng(5).integers(0, 256, shape + (4,)).astype(np.uint8)
    once = tw.rgba_render_runs("plain", gs, places, cols, runs, None, out.copy(), 4, True, load=True)
    twice = tw.rgba_render_runs("plain", gs, places, cols, runs, None, once.copy(), 4, True, load=True)
    assert not np.array_equal(once, twice)


@pytest.mark.parametrize("data", [np.zeros((5, 4), np.uint8), np.zeros((6, 3), np.uint8), np.zeros((6, 4), np.int32),
                                  np.zeros((2, 3, 4), np.uint8), [[0, 0, 0, 0]] * 6])
def test_draw_text_rgba_rejects_a_mismatched_image(data):
    """the image's pixels must be exactly (height * width, 4) u8 before anything goes to the device"""
    font = load_font("DejaVuSans.ttf", allow_hinted=True)
    with pytest.raises(ValueError):
        fr.draw_text_rgba(fr.RGBA(3, 2, data), font, "A", 20, 0, 10)

"""The colour arithmetic of the RGBA text kernels over its whole domain, on the device (tests/text_block_cases.py): every
(C, c, A) of the blend, every (k, C, c) of the opaque resolve, two layers and the walk over hidden samples.  The geometry
is cover(k, W, n) at the centre phase, so every pixel's coverage is known without a twin, and every expected byte is the
integer formula of include/fr_raster.h (for FR_TEXT_SRGB through the tables D / E of the IEC decode).  Buffers carry a
sentinel border; the whole array is compared with np.array_equal."""
from contextlib import closing
from functools import lru_cache

import numpy as np
import pytest

import font_renderer_amd as fr
import text_block_cases as B
import text_gpu as G
from text_gpu import BGRA, FILL, LOAD, SRGB

pytestmark = pytest.mark.gpu
FORMS = [False, True]                                          # fr_glyph_place, fr_glyph_place_ex


def _name(ex, srgb, load, n, fill, blend):
    return "fr::text_%s%s%skernel<%d, %d, %d>" % ("place_" if ex else "", "srgb_" if srgb else "rgba_", "load_" if load else "",
                                                  n, 1 if fill else 0, blend)


def _run(ctx, case, n, flags, name):
    """render the case over a device copy of its start buffer, assert the kernel instance, compare every byte"""
    info = {}
    with closing(fr.DeviceGlyphSet(ctx, B.glyph_set(case.glyphs))) as dgs:
        got = G.render_rgba(ctx, dgs, case.places, case.rgba, case.runs, case.clears, case.start, n, True, flags, info=info)
    assert name in info["describe"], (name, info)
    if not np.array_equal(got, case.want):
        bad = np.argwhere((got != case.want).any(axis=-1))
        y, x = bad[0]
        raise AssertionError("%s: %d pixels differ, first at (%d, %d): got %s, want %s, start %s"
                             % (name, len(bad), y, x, got[y, x], case.want[y, x], case.start[y, x]))


@lru_cache(maxsize=2)
def _blend_load(srgb, bgra):
    """the 22.5 MB expectation depends on neither n nor the placement form: the resolve of equal samples is the identity"""
    return B.blend_load_case(4, False, srgb, bgra)


def _with_form(case, n, ex):
    """the shared expectation with the glyph of this n and the placements in this form"""
    places = case.places
    if ex:
        places = np.zeros(len(case.places), B.rg.PLACE_EX_DTYPE)
        places["glyph"], places["pen_x64"], places["pen_y64"] = case.places["glyph"], case.places["pen_x64"], 64 * case.places["pen_y"]
    return B.ColourCase(**{**case.__dict__, "places": places, "glyphs": [B.cover(n * n, 86, n)]})


@pytest.mark.parametrize("n", [1, 2, 4])
@pytest.mark.parametrize("srgb", [False, True], ids=["unorm", "srgb"])
@pytest.mark.parametrize("ex", FORMS, ids=["place", "place_ex"])
def test_blend_over_loaded_pixels_every_C_c_A(ctx, ex, srgb, n):
    """65 536 translucent blocks, one per (C, A), over pixels that run through every c: all 16.7 M triples per channel"""
    flags = LOAD | (SRGB if srgb else 0)
    _run(ctx, _with_form(_blend_load(srgb, False), n, ex), n, flags, _name(ex, srgb, True, n, 0, 1))


@pytest.mark.parametrize("ex,srgb,n,extra", [(False, True, 4, FILL), (True, False, 2, FILL), (False, False, 4, BGRA), (True, True, 1, BGRA)])
def test_blend_over_loaded_pixels_fill_and_bgra(ctx, ex, srgb, n, extra):
    flags = LOAD | (SRGB if srgb else 0) | extra
    case = _with_form(_blend_load(srgb, extra == BGRA), n, ex)
    _run(ctx, case, n, flags, _name(ex, srgb, True, n, extra == FILL, 1))


@pytest.mark.parametrize("srgb", [False, True], ids=["unorm", "srgb"])
@pytest.mark.parametrize("ex", FORMS, ids=["place", "place_ex"])
def test_blend_over_clear_colours(ctx, ex, srgb):
    """the same (C, A) pairs over 256 clear colours: every pair out of C, c and A, n = 1, 2, 4"""
    for n in (1, 2, 4):
        fill = FILL if n == 2 else 0
        _run(ctx, B.blend_clear_case(n, ex, srgb), n, (SRGB if srgb else 0) | fill, _name(ex, srgb, False, n, fill, 1))


@pytest.mark.parametrize("srgb", [False, True], ids=["unorm", "srgb"])
@pytest.mark.parametrize("ex", FORMS, ids=["place", "place_ex"])
def test_opaque_resolve_every_k_C_c(ctx, ex, srgb):
    """BLEND = 0: k samples of the opaque colour C and n^2 - k of the pixel already there, every (k, C, c); k = 0 is the
    pixel no instance touches (under FR_TEXT_LOAD the store-skip path); then every (C, c) over clear colours"""
    for n in (1, 2, 4):
        fill = FILL if n == 1 else 0
        flags = (SRGB if srgb else 0) | fill
        _run(ctx, B.opaque_load_case(n, ex, srgb), n, flags | LOAD, _name(ex, srgb, True, n, fill, 0))
        _run(ctx, B.opaque_clear_case(n, ex, srgb), n, flags, _name(ex, srgb, False, n, fill, 0))


@pytest.mark.parametrize("srgb", [False, True], ids=["unorm", "srgb"])
@pytest.mark.parametrize("ex", FORMS, ids=["place", "place_ex"])
def test_two_layers(ctx, ex, srgb):
    """a translucent placement over a translucent placement on a 64 x 64 lattice of (A1, A2): the sample state is stored
    (for sRGB encoded and decoded again) between the blends; and an opaque cover(k2) over an opaque cover(k1) for every
    (k1, k2): the walk over the samples already taken"""
    for n in (1, 2, 4):
        flags = SRGB if srgb else 0
        _run(ctx, B.two_layer_case(n, ex, srgb), n, flags | LOAD, _name(ex, srgb, True, n, 0, 1))
        for load in (False, True):
            _run(ctx, B.opaque_overlap_case(n, ex, srgb, load), n, flags | (LOAD if load else 0), _name(ex, srgb, load, n, 0, 0))

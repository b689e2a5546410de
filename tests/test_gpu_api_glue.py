"""GPU suite: the glue of the C ABI units (csrc/fr_api_*.hip) that no kernel test reaches on its own — fr_render_glyph's
launches over views of its arena against a plan of the same one job, and who owns device memory (create / destroy cycles
must give back every byte)."""

import numpy as np
import pytest

import font_renderer_amd as fr
import text_instance_cases as T
from font_renderer_amd import _lib as L
from font_renderer_amd import render_glyph as rg
from font_renderer_amd.glyph import Box, Contour, Glyph, GlyphSet
from font_renderer_amd.synth import synth_glyph, synth_glyphset

pytestmark = pytest.mark.gpu

MODES = (fr.FR_GRAY_DEBUG, fr.FR_MASK_NONZERO, fr.FR_COVERAGE_U8, fr.FR_WINDING_I16, fr.FR_SDF_U8)


def _render_glyph(ctx, glyph, upm, size, mode, flags, shape):
    out = np.zeros(shape, np.int16 if mode == fr.FR_WINDING_I16 else np.uint8)
    gs = GlyphSet([glyph])
    box = glyph.box.as_array()
    L.check(ctx._lib.fr_render_glyph_ex(ctx._h, L.ptr(gs.points_xy), L.ptr(gs.contour_start), gs.n_contours, L.ptr(box), upm, size, mode, flags,
                                        L.ptr(out)))
    return out


def test_single_glyph_equals_plan_of_its_one_job(ascii_set):
    """fr_render_glyph == fr_render_batch of the one job fr_render_glyph_dims gives, byte for byte: STIX 'A' at 64
    (47 x 45: records built in the kernel) and a synthetic glyph of 200 segments (records staged by prepare_kernel behind
    the count memset), every mode the entry point takes, both fill rules.  The calls alternate between the glyphs in a
    context of their own, so the arena is reused, and the big glyph's winding image (2 bytes per pixel, more than the
    arena's first 1 MiB) makes it grow in the middle of the sequence."""
    i = ascii_set.find("STIX", "A")
    cs, box = synth_glyph(5, 200)
    big = Glyph(Box(*(int(v) for v in box)), [Contour(c) for c in cs])
    cases = [(ascii_set.glyph(i), int(ascii_set.g_upm[i]), 64), (big, 2048, 1200)]
    with fr.Context(0) as ctx:
        sets = [fr.DeviceGlyphSet(ctx, GlyphSet([g])) for g, _, _ in cases]
        grown = 0
        for mode in MODES:
            for flags in (0, fr.FR_FILL_CONSISTENT):
                for (glyph, upm, size), dgs in zip(cases, sets):
                    mn, mx, w, h, scale = rg.render_glyph_dims(glyph.box.as_array(), upm, size)
                    if glyph is not big:
                        assert (w, h) == (47, 45)
                    grown += w * h * 2 > (1 << 20) and mode == fr.FR_WINDING_I16
                    got = _render_glyph(ctx, glyph, upm, size, mode, flags, (h, w))
                    want = np.zeros_like(got)
                    rg.render_batch(dgs, rg.make_jobs([(0, mn[0], mx[1], w, h, 0, 0, scale)]), mode, want, 1, fr.FR_SAMPLE_CORNER, flags)
                    assert want.any()
                    assert np.array_equal(got, want), (mode, flags, size)
        assert grown == 2
        for dgs in sets:
            dgs.close()


def _free_bytes():
    import torch
    torch.cuda.synchronize()
    return torch.cuda.mem_get_info()[0]


# D(200) - D(20) of the library before device memory had one owner, measured with this loop
PARENT_GROWTH = 0


def test_create_destroy_cycles_give_device_memory_back(ctx, ascii_set):
    """create / destroy cycles of a tiny glyph set, an SDF raster plan (with bit planes), a plain text plan and an
    FR_TEXT_CACHE text plan: D(k), the drop in free device memory after k cycles, grows no more from 20 to 200 cycles than
    it did in the library whose destroy functions freed by list"""
    tiny = synth_glyphset(2, 8)
    sdf_set = synth_glyphset(2, 64)
    jobs = rg.make_jobs([(g, 0, 64, 64, 64, 64 * g, 0, 64.0 / 2048.0) for g in range(2)])
    text_set = T.glyph_set(ascii_set)
    dgs, tgs = fr.DeviceGlyphSet(ctx, sdf_set), fr.DeviceGlyphSet(ctx, text_set)
    probe = fr.Plan(dgs, jobs, fr.FR_SDF_U8, 1, fr.FR_SAMPLE_CENTER)
    assert "win1_kernel" in probe.describe(), probe.describe()          # the fast kernels' sign pass: the plan has bit planes
    probe.close()

    def cycle():
        fr.DeviceGlyphSet(ctx, tiny).close()
        fr.Plan(dgs, jobs, fr.FR_SDF_U8, 1, fr.FR_SAMPLE_CENTER).close()
        for flags in (0, fr.FR_TEXT_CACHE):
            fr.TextPlan(tgs, T.places_of(0), T.runs(), fr.FR_COVERAGE_U8, 4, fr.FR_SAMPLE_CORNER, flags).close()

    cycle()                                                              # (whatever the first use of a code path keeps)
    free0 = _free_bytes()
    drop = {}
    for k in range(1, 201):
        cycle()
        if k in (20, 200):
            drop[k] = free0 - _free_bytes()
    print(f"D(20) = {drop[20]} bytes, D(200) = {drop[200]} bytes")
    dgs.close(); tgs.close()
    assert drop[200] - drop[20] <= PARENT_GROWTH, drop

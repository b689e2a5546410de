"""The launch list of a raster plan (csrc/fr_raster_plan.cpp) on the GPU: the smallest plans in which the fork, the join,
the bit plane and the second prepare all occur.  Two fast parts (64 cells of 20 x 20 and 64 of 70 x 20) and one cell of
16 x 520 of a 200-segment glyph, which at 4 x 4 samples is the general kernel's (2 080 sample rows) and needs
prepare_kernel: as coverage, as FR_SDF_U8 and under FR_FILL_CONSISTENT.  fr_plan_describe must return exactly the string
tests/golden/raster_plan_describe.json holds — minted from the library as it was before the plan rules left fr_api.hip —
and a render with option overlap = 0 and = 2 must equal the CPU reference byte for byte.
Option kmax picks the CAP instance (raster_launches): a plan of two 20 x 20 coverage cells under kmax on both sides of 8, 16
and 32, on the fast kernels and on the general one, must be described as the library described it while the launch
functions still chose the instance (the golden file's "kmax<k>/cov4_<c>" strings), and must render the same bytes under
every kmax."""
import functools
import json
import os

import numpy as np
import pytest

import fill_rule_ref
import font_renderer_amd as fr
import oracle_lib as O
from font_renderer_amd import render_glyph as rg
from font_renderer_amd.atlas import cell_jobs
from font_renderer_amd.glyph import GlyphSet
from font_renderer_amd.synth import synth_glyphset

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "raster_plan_describe.json")
SHAPE = (524, 1181)
SENT = 0x5b
# name -> (mode, the oracle's mode, samples per axis, flags, jobs on the general kernel: at one sample per pixel the tall
# cell's 520 sample rows fit win1_kernel)
PLANS = {"coverage": (fr.FR_COVERAGE_U8, O.COVERAGE_U8, 4, 0, 1), "sdf": (fr.FR_SDF_U8, O.SDF_U8, 1, 0, 0),
         "fill": (fr.FR_COVERAGE_U8, O.COVERAGE_U8, 4, fr.FR_FILL_CONSISTENT, 1)}


@functools.lru_cache(maxsize=None)
def glyphs_and_jobs():
    parts = [synth_glyphset(2, 40, first_index=31), synth_glyphset(1, 200, first_index=32)]
    gs = GlyphSet([p.glyph(i) for p in parts for i in range(len(p))])
    small, tall = cell_jobs(gs, 20, 18, 2048, 3), cell_jobs(gs, 520, 500, 2048, 3)      # origin and scale of each glyph at a size
    jobs = np.zeros(129, small.dtype)
    i = np.arange(64)
    jobs[:64], jobs[64:128], jobs[128] = small[0], small[1], tall[2]
    jobs["w"][:64], jobs["h"][:64], jobs["out_x"][:64], jobs["out_y"][:64] = 20, 20, 1 + (i % 16) * 23, 2 + (i // 16) * 22
    jobs["w"][64:128], jobs["h"][64:128], jobs["out_x"][64:128], jobs["out_y"][64:128] = 70, 20, 3 + (i % 16) * 72, 100 + (i // 16) * 21
    jobs["w"][128], jobs["h"][128], jobs["out_x"][128], jobs["out_y"][128] = 16, 520, 1162, 1
    return gs, jobs


@functools.lru_cache(maxsize=None)
def reference(oracle, name):
    gs, jobs = glyphs_and_jobs()
    mode, omode, n, flags, _ = PLANS[name]
    ref = np.full(SHAPE, SENT, np.uint8)
    if flags:
        fill_rule_ref.render_batch(gs, jobs, mode, ref, n, True)
    else:
        oracle.render_batch(gs, jobs, omode, ref, n, True, 16)
    ref.setflags(write=False)
    return ref


def describe(ctx, dgs, name):
    mode, _, n, flags, _ = PLANS[name]
    plan = fr.Plan(dgs, glyphs_and_jobs()[1], mode, n, fr.FR_SAMPLE_CENTER, flags)
    text, stats = plan.describe(), plan.stats()
    plan.close()
    return text, stats


@pytest.mark.parametrize("name", list(PLANS))
def test_describe_is_the_parents_and_both_stream_layouts_render_the_reference(ctx, oracle, name):
    gs, jobs = glyphs_and_jobs()
    mode, _, n, flags, n_general = PLANS[name]
    with open(GOLDEN) as f:
        want = json.load(f)[name]
    dgs = fr.DeviceGlyphSet(ctx, gs)
    try:
        text, stats = describe(ctx, dgs, name)
        assert text == want
        assert stats == {"jobs_cov4": 129 - n_general, "jobs_general": n_general}
        ref = reference(oracle, name)
        assert (ref != SENT).any()
        for overlap in (0, 2):
            ctx.set_option("overlap", overlap)
            got = np.full(SHAPE, SENT, np.uint8)
            rg.render_batch(dgs, jobs, mode, got, n, fr.FR_SAMPLE_CENTER, flags)
            assert np.array_equal(got, ref), (name, overlap, text)
    finally:
        ctx.set_option("overlap", 1)                       # (the default; the library has no call that reads an option back)
        dgs.close()


KMAX = (1, 8, 9, 16, 17, 32, 128)
KMAX_SHAPE = (24, 47)


def kmax_jobs():
    """two 20 x 20 cells, one of each 40-segment glyph"""
    jobs = glyphs_and_jobs()[1][[0, 64]].copy()
    jobs["w"], jobs["h"], jobs["out_x"], jobs["out_y"] = 20, 20, (1, 24), 2
    return jobs


def test_describe_under_every_kmax_is_the_parents_and_the_renders_are_one(ctx, oracle):
    gs, jobs = glyphs_and_jobs()[0], kmax_jobs()
    with open(GOLDEN) as f:
        want = json.load(f)
    ref = np.full(KMAX_SHAPE, SENT, np.uint8)
    oracle.render_batch(gs, jobs, O.COVERAGE_U8, ref, 4, True)
    assert (ref != SENT).any() and (ref[0] == SENT).all() and (ref[:, 0] == SENT).all()
    dgs = fr.DeviceGlyphSet(ctx, gs)
    try:
        for cov4 in (1, 0):
            ctx.set_option("cov4", cov4)
            got = {}
            for kmax in KMAX:
                ctx.set_option("kmax", kmax)
                plan = fr.Plan(dgs, jobs, fr.FR_COVERAGE_U8, 4, fr.FR_SAMPLE_CENTER, 0)
                text, stats = plan.describe(), plan.stats()
                plan.close()
                assert text == want[f"kmax{kmax}/cov4_{cov4}"], (kmax, cov4)
                assert stats == ({"jobs_cov4": 2, "jobs_general": 0} if cov4 else {"jobs_cov4": 0, "jobs_general": 2})
                got[kmax] = np.full(KMAX_SHAPE, SENT, np.uint8)
                rg.render_batch(dgs, jobs, fr.FR_COVERAGE_U8, got[kmax], 4, fr.FR_SAMPLE_CENTER, 0)
            for kmax in KMAX:
                assert np.array_equal(got[kmax], got[32]), (kmax, cov4)
                assert np.array_equal(got[kmax], ref), (kmax, cov4)
    finally:
        ctx.set_option("kmax", 32)                         # (the defaults)
        ctx.set_option("cov4", 1)
        dgs.close()

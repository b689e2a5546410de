"""What the GPU text test modules (tests/test_gpu_text*.py) share: rendering a text plan into a prepared device buffer,
reading its launches, the noise, colours and border checks of their cases, and the one dispatch from a plan's flags to
its CPU twin (tests/text_twin.py).  A plain helper module, imported like fixtures.py."""
import re
from contextlib import closing

import numpy as np
import pytest

import font_renderer_amd as fr
import text_twin as tw
from fixtures import load_font
from font_renderer_amd import render_glyph as rg

FILL, SRGB, BGRA, LOAD, CACHE, OVER = (fr.FR_FILL_CONSISTENT, fr.FR_TEXT_SRGB, fr.FR_TEXT_BGRA, fr.FR_TEXT_LOAD, fr.FR_TEXT_CACHE,
                                       fr.FR_TEXT_OVER)
FORM_NAME = {"plain": "", "ex": "place_", "affine": "affine_"}


def phase(center):
    return fr.FR_SAMPLE_CENTER if center else fr.FR_SAMPLE_CORNER


def _render(ctx, plan, buf, times, info):
    """`plan` rendered `times` times into the device tensor `buf`, then closed -> the bytes (host)"""
    import torch
    with closing(plan):
        torch.cuda.synchronize()
        for _ in range(times):
            plan.render(buf.data_ptr(), buf.shape[1], buf.shape[0])
        ctx.sync()
        if info is not None:
            info.update(describe=plan.describe(), stats=plan.stats(), pixels=plan.pixels)
    return buf.cpu().numpy()


def render_gray(ctx, dgs, places, runs, shape, mode=fr.FR_COVERAGE_U8, n=4, center=True, flags=0, *, sent=0x5b, times=1, info=None):
    """a coverage / mask plan of any placement form into a buffer filled with `sent` -> the bytes; info, when given,
    receives describe, stats and pixels of the plan"""
    import torch
    plan = fr.TextPlan(dgs, places, runs, mode, n, phase(center), flags)
    return _render(ctx, plan, torch.full(shape, sent, dtype=torch.uint8, device="cuda:0"), times, info)


def render_rgba(ctx, dgs, places, cols, runs, clears, dst, n=4, center=True, flags=0, *, times=1, info=None):
    """an RGBA plan of any placement form over a device copy of dst ((rows, cols, 4) u8: a sentinel, or noise under
    FR_TEXT_LOAD) -> the bytes; info as in render_gray"""
    import torch
    plan = fr.TextPlanRGBA(dgs, places, cols, runs, clears, n, phase(center), flags)
    return _render(ctx, plan, torch.from_numpy(np.ascontiguousarray(dst)).to("cuda:0"), times, info)


def sent4(shape, sent):
    """a (rows, cols, 4) u8 buffer holding the byte or the four-byte pattern `sent` in every pixel"""
    out = np.empty(shape + (4,), np.uint8)
    out[:] = sent
    return out


def count(describe, kernel):
    """the count fr_plan_describe reports for `kernel`"""
    m = re.search(re.escape(kernel) + r" x(\d+)", describe)
    assert m, (kernel, describe)
    return int(m.group(1))


def kernel_name(form, flags, n, blend):
    return "fr::text_%s%s%skernel<%d, %d, %d> x" % (FORM_NAME[form], "srgb_" if flags & SRGB else "rgba_", "load_" if flags & LOAD else "",
                                                     n, 1 if flags & FILL else 0, blend)


def cached_kernel_name(flags, n, blend):
    return "fr::text_cached_%s%skernel<%d, %d> x" % ("srgb_" if flags & SRGB else "rgba_", "load_" if flags & LOAD else "", n, blend)


def noise(shape, seed):
    return np.random.default_rng(seed).integers(0, 256, shape + (4,)).astype(np.uint8)


def colours(n, seed, opaque):
    c = np.random.default_rng(seed).integers(0, 256, (n, 4)).astype(np.uint8)
    if opaque:
        c[:, 3] = 255
    else:
        c[::3, 3] = 255                                                   # a mix: opaque, translucent, and one clear glyph
        c[1 % n, 3] = 0
    return c


def inside(runs, shape):
    m = np.zeros(shape, bool)
    for r in runs:
        m[r["out_y"]:r["out_y"] + r["h"], r["out_x"]:r["out_x"] + r["w"]] = True
    return m


def check_borders(got, runs, sent):
    """every pixel outside the runs holds the four-byte sentinel, and none inside does"""
    is_sent = (got == sent).all(axis=2)
    m = inside(runs, got.shape[:2])
    assert is_sent[~m].all() and not is_sent[m].any()


def degenerate(places, scale=0.0):
    """fr_glyph_place rows as fr_glyph_place_ex: pen_y64 = 64 pen_y, scale 0 (or the given one), slant 0"""
    return rg.make_places_ex([(int(p["glyph"]), int(p["pen_x64"]), 64 * int(p["pen_y"]), scale, 0.0) for p in places])


def twin_gray(form, gs, places, runs, shape, n=4, center=True, fill=False, which=None, *, sent=0x5b):
    """what render_gray must give: the twin's runs in a buffer filled with `sent`"""
    return tw.render_runs(form, gs, places, runs, np.full(shape, sent, np.uint8), n, center, bool(fill), which)


def twin_rgba(form, gs, places, cols, runs, clears, dst, n=4, center=True, flags=0, which=None):
    """what render_rgba must give for the plan's flags, over a copy of dst"""
    args = (n, center, bool(flags & FILL), bool(flags & SRGB), bool(flags & BGRA), bool(flags & LOAD))
    if flags & OVER:
        assert which is None
        return tw.over_render_runs(form, gs, places, cols, runs, clears, dst, *args)
    return tw.rgba_render_runs(form, gs, places, cols, runs, clears, dst.copy(), *args, which)


@pytest.fixture(scope="module")
def italic():
    """three italic lines at size 21, the third a run of glyphs packed so close that their ink overlaps"""
    font = load_font("DejaVuSerif-Italic.ttf")
    gs, places, runs, shape = tw.lines(font, ["ffi fj Tf ff", "Tjfyfgf jjj", "WoWfj"], 21, pad=2)
    k0 = int(runs[2]["first"])
    places["pen_x64"][k0:k0 + 5] = places["pen_x64"][k0] + np.array([0, 213, 410, 641, 817])
    return gs, places, runs, shape

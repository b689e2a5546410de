"""CPU twin of FR_TEXT_LOAD text plans (fr_text_plan_create_rgba with FR_TEXT_LOAD, include/fr_raster.h, DESIGN.md
section 5), written from the definition and not from the kernel: every sub-sample of a pixel starts at the pixel's value
in the output (the pixel repeated n x n), and then the per-instance non-zero tests of tests/text_rgba_ref.instance_hits
are applied in placement order with the blend and resolve of tests/text_rgba_ref.py (UNORM) or tests/text_srgb_ref.py
(FR_TEXT_SRGB, whose D and E decode and encode the stored bytes).  FR_TEXT_BGRA reads and writes the element as B G R A:
the pixels are swapped to R G B A before the computation and back after it."""
import numpy as np

import text_rgba_ref as tr
import text_srgb_ref as ts


def run_samples(gs, places, place_rgba, run, dst, n=1, center=False, fill=False, srgb=False):
    """dst: the run's (h, w, 4) pixels, R G B A -> (h n, w n, 4) int64: every sub-sample after the run's instances"""
    smp = np.repeat(np.repeat(np.asarray(dst, np.int64), n, axis=0), n, axis=1)
    blend = ts.blend if srgb else tr.blend
    for k, y0, x0, hit in tr.instance_hits(gs, places, run, n, center, fill):
        view = smp[y0 * n:y0 * n + hit.shape[0], x0 * n:x0 * n + hit.shape[1]]
        view[hit] = blend(view[hit], place_rgba[k])
    return smp


def render_run(gs, places, place_rgba, run, dst, n=1, center=False, fill=False, srgb=False, bgr=False):
    """the run's pixels after a render over dst (both (h, w, 4) u8, in the stored byte order)"""
    d = ts.bgra(dst) if bgr else dst
    smp = run_samples(gs, places, place_rgba, run, d, n, center, fill, srgb)
    img = ts.resolve(smp, n) if srgb else tr.resolve(smp, n)
    return ts.bgra(img) if bgr else img


def render_runs(gs, places, place_rgba, runs, out, n=1, center=False, fill=False, srgb=False, bgr=False, which=None):
    """every run (or the runs `which`) drawn over the (rows, cols, 4) u8 array `out`, in place, as a LOAD plan draws it"""
    for r in (range(len(runs)) if which is None else which):
        run = runs[r]
        oy, ox, h, w = int(run["out_y"]), int(run["out_x"]), int(run["h"]), int(run["w"])
        if not w or not h:
            continue
        sl = np.s_[oy:oy + h, ox:ox + w]
        out[sl] = render_run(gs, places, place_rgba, run, out[sl].copy(), n, center, fill, srgb, bgr)
    return out

"""Text-run benchmark: 4 096 lines of 64 printable ASCII characters, one run per line, one plan,
4 x 4 samples (--samples), for DejaVuSans and DejaVuSerif-Italic at font sizes 16 and 32.  Reports per configuration the ms per render
of the text plan and its Mpixel/s of run area, and the same instances as separate cells (renderGlyph's grid, whole-pixel
origins, disjoint) in a plain plan, which prices the composition.  Under rocprofv3 --kernel-trace --stats the kernel
shares come from the trace (prepare_kernel vs text_kernel).  Prints one JSON line per configuration.

--rgba adds the same lines as RGBA text plans (fr_text_plan_create_rgba), which prices colour against the coverage plan
on the same box: alternating per-word colours, all opaque (text_rgba_kernel<4, 0, 0>), and the same with the first line
in translucent colours (so the plan blends: text_rgba_kernel<4, 0, 1>).

--srgb adds the same two colourings as sRGB text plans (FR_TEXT_SRGB: blending and resolve in linear light,
text_srgb_kernel<4, 0, 0> / <4, 0, 1>), priced against the coverage plan (and the RGBA plans, with --rgba) in the same run.

--load adds FR_TEXT_LOAD (text drawn over the pixels already in the output): (a) the same lines and colourings as LOAD
plans over a noise background, UNORM and sRGB (text_rgba_load_kernel / text_srgb_load_kernel), priced against the
clear-colour plans of the same kind in the same run; (b) a sparse overlay, printed as its own JSON line: 16 lines of 64
characters at size 32 on a 3840 x 2160 frame as one LOAD run covering the frame, against the same placements in one
clear-colour run over the whole frame.  Every render of a LOAD plan, warm-up included, starts from a fresh device copy of
the noise in a buffer of its own (the copy is outside the timed region); the clear-colour plans render into another
buffer, after the same copy.  "tiles_load_computed" is the tile count recomputed here from the clipped cells, not observed: the launched
grid is what a rocprofv3 --kernel-trace run shows (e.g. of --load --lines 1).

--place prices the placement form (fr_text_plan_create_ex / _rgba_ex: own scale, slant and sub-pixel baseline per
placement), printed as its own JSON lines ("case": "place"), one per font and size, for the coverage plan and the RGBA plan
with opaque and with translucent colours: (a) the plan of the old entry point, (b) the _ex plan with degenerate
parameters — the same pixels and records through the wider instance record —, (c) the _ex plan with slant 0.2 and a
random baseline fraction per placement.  The three are timed alternately in the same process, --repeats times over;
each figure is the median over the repeats of the median of --steps renders, with the smallest and largest repeat of
(a) beside it: a difference of (b) from (a) inside that spread is not a difference.  (b) must render (a)'s bytes (checked).

--affine prices the matrix form (fr_text_plan_create_affine: a 2 x 2 matrix per placement, every lane solving every
record at its own ray height, fr_text_affine.hip), printed as its own JSON lines ("case": "affine"), one per font and
size, coverage plans: (a) the _ex plan of the lines, (b) the affine plan at 0 degrees, where the kernel's cull removes
nearly every record, (c) at 5, (d) at 45 and (e) at 90 degrees, where a wave's row spans the glyph's whole height and
the cull removes nothing.  Every line keeps a run of its own, as large as the union of its rotated cells (so at 45
degrees the runs are squares around a diagonal line: "run_mpixel" is reported per form), shelf-packed into one image.
The five are timed alternately in the same process, --repeats times over; figures as for --place.  --affine-only
leaves the other configurations out.

--cache prices FR_TEXT_CACHE (one mask cell per distinct (glyph, pen fraction, scale), filled once per render and read by
every instance of the key: csrc/fr_text_cached.hip), printed as its own JSON lines ("case": "cache"), one per font and
size, coverage plans: (a) the plain plan, (b) the same plan with the flag, timed alternately in the same process,
--repeats times over; figures as for --place, so "a_min_ms" .. "a_max_ms" is the plain plan's own run-to-run spread.  (b)
must render (a)'s bytes (checked).  Beside the times: instances and cells (from fr_plan_describe), the mask store's
bytes (recomputed here from the cells), and as the kernel split "cells_only_ms": a plain plan that holds every key's
placement exactly once, each in a run of its cell's size — the prepare kernel and the direct sum over every distinct
glyph image once, which is the work of the cached plan's first two launches; the composite is what remains of (b).
--cache-only leaves the other configurations out.

--affine --cache together price the mask cache of the matrix form instead of those two: the five variants of --affine, each
as its plain plan and as its cached plan (FR_TEXT_CACHE for the _ex plan (a), FR_TEXT_CACHE_AFFINE for (b)-(e)), the ten
alternated in the same process, --repeats times; the two images of a variant must be equal.  One JSON line per font and
size ("case": "affine_cache") with, per variant, the instances, the cells, the bytes of the mask store and both medians
with their smallest and largest repeat.

--over prices FR_TEXT_OVER (source-over alpha: the colour kernels' third blend value, csrc/fr_text_colour_kernel.inc),
printed as its own JSON lines ("case": "over"), one per font and size: the --rgba translucent colouring as (a) the plan
without the flag (blend = 1) and (b) the plan with it (blend = 2), UNORM and sRGB, timed alternately in the same process,
--repeats times over; figures as for --place, so "a_min_ms" .. "a_max_ms" is the flag-less plan's own run-to-run spread.
(b) must render (a)'s R, G and B (checked).  --over-only leaves the other configurations out.

--samples {1,2,4} (default 4) and --fill (FR_FILL_CONSISTENT) go to every plan, so the kernel instances named below as
<4, 0, ...> become <samples, fill, ...>.  The text kernels live in csrc/fr_text.hip, those of the matrix form in
csrc/fr_text_affine.hip.

    python tools/bench_text.py [--lines 4096] [--chars 64] [--steps 20] [--warmup 3] [--samples 4] [--fill]
                               [--rgba] [--srgb] [--load]
                               [--place [--repeats 5] [--place-only]] [--affine [--affine-only]]
                               [--cache [--cache-only]] [--over [--over-only]]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import font_renderer_amd as fr  # noqa: E402
from font_renderer_amd import render_glyph as rg  # noqa: E402
from fixtures import load_font  # noqa: E402


def workload(font, n_lines, n_chars, size, seed):
    rng = np.random.default_rng(seed)
    alphabet = [chr(c) for c in range(0x20, 0x7f)]
    lines = ["".join(rng.choice(alphabet, n_chars)) for _ in range(n_lines)]
    lay = [font.layout(s, size) for s in lines]
    distinct = sorted({int(g) for gi, _, _ in lay for g in gi})
    gs, kept = font.glyphset(distinct, skip_unsupported=False)
    local = {g: k for k, g in enumerate(kept)}
    scale = np.float32(size) / np.float32(font.information.units_per_em)
    seg = gs.segments_per_glyph()
    places, runs, jobs = [], [], []
    y, W, jy, JW = 0, 0, 0, 0
    for gi, pen, _ in lay:
        cells = [fr.instance_cell(gs.boxes[local[int(g)]], scale, int(p), 0) for g, p in zip(gi, pen) if seg[local[int(g)]]]
        left, top = min(c[0] for c in cells), min(c[1] for c in cells)
        shift = max(-left, 0)
        w = max(c[0] + c[2] for c in cells) + shift
        h = max(c[1] + c[3] for c in cells) - top
        runs.append((len(places), len(gi), w, h, 0, y, scale))
        places += [(local[int(g)], int(p) + 64 * shift, -top) for g, p in zip(gi, pen)]
        y += h
        W = max(W, w)
        # the same instances as plain jobs: renderGlyph's grid, side by side on a row of their own
        x, jh = 0, 0
        for g, p in zip(gi, pen):
            if not seg[local[int(g)]]:
                continue
            c0, r0, cw, ch = fr.instance_cell(gs.boxes[local[int(g)]], scale, 0, 0)
            jobs.append((local[int(g)], c0, -r0, cw, ch, x, jy, scale))
            x += cw
            jh = max(jh, ch)
        jy += jh
        JW = max(JW, x)
    return gs, rg.make_places(places), rg.make_runs(runs), (y, W), rg.make_jobs(jobs), (jy, JW), lines


def timed_over(plan, buf, src, shape, steps, warmup):
    """the median ms of `steps` renders into buf, after `warmup`, each starting from a fresh copy of src (not timed)"""
    import torch
    ms = []
    for i in range(warmup + steps):
        buf.copy_(src)
        torch.cuda.synchronize()
        t = plan.render_timed(buf.data_ptr(), shape[1], shape[0])
        if i >= warmup:
            ms.append(t)
    ms.sort()
    return ms[len(ms) // 2]


def timed(plan, buf, shape, steps, warmup):
    for _ in range(warmup):
        plan.render_timed(buf.data_ptr(), shape[1], shape[0])
    ms = sorted(plan.render_timed(buf.data_ptr(), shape[1], shape[0]) for _ in range(steps))
    return ms[len(ms) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lines", type=int, default=4096)
    ap.add_argument("--chars", type=int, default=64)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rgba", action="store_true", help="also render the lines as RGBA text plans")
    ap.add_argument("--srgb", action="store_true", help="also render the lines as sRGB (linear-light) RGBA text plans")
    ap.add_argument("--load", action="store_true", help="also draw the lines over a noise background (FR_TEXT_LOAD), each "
                    "render from a fresh copy of it, and a sparse overlay on a 3840 x 2160 noise frame")
    ap.add_argument("--samples", type=int, choices=(1, 2, 4), default=4, help="samples per axis of every plan")
    ap.add_argument("--fill", action="store_true", help="build every plan with FR_FILL_CONSISTENT")
    ap.add_argument("--place", action="store_true", help="also price the placement form (fr_glyph_place_ex) against the old "
                    "entry points, alternating in the same run")
    ap.add_argument("--repeats", type=int, default=5, help="--place: repeats of each alternated timing (at least 5)")
    ap.add_argument("--place-only", action="store_true", help="--place without the other configurations")
    ap.add_argument("--affine", action="store_true", help="also price the matrix form (fr_glyph_place_affine) at 0, 5, 45 and 90 "
                    "degrees against the _ex plan, alternating in the same run (--repeats)")
    ap.add_argument("--affine-only", action="store_true", help="--affine without the other configurations")
    ap.add_argument("--cache", action="store_true", help="also price FR_TEXT_CACHE against the plain plan, alternating in the "
                    "same run (--repeats)")
    ap.add_argument("--cache-only", action="store_true", help="--cache without the other configurations")
    ap.add_argument("--over", action="store_true", help="also price FR_TEXT_OVER against the plan without it, UNORM and sRGB, "
                    "alternating in the same run (--repeats)")
    ap.add_argument("--over-only", action="store_true", help="--over without the other configurations")
    args = ap.parse_args()
    if (args.place or args.affine or args.cache or args.over) and args.repeats < 5:
        ap.error("--repeats: at least 5")
    import torch
    ns, fill = args.samples, fr.FR_FILL_CONSISTENT if args.fill else 0
    ctx = fr.Context(0)
    if args.place:
        place(ctx, args)
    if args.affine and args.cache:
        affine_cache(ctx, args)
    elif args.affine:
        affine(ctx, args)
    elif args.cache:
        cache(ctx, args)
    if args.over:
        over(ctx, args)
    only = ((args.place and args.place_only) or (args.affine and args.affine_only) or (args.cache and args.cache_only)
            or (args.over and args.over_only))
    for fi, name in enumerate([] if only else ["DejaVuSans.ttf", "DejaVuSerif-Italic.ttf"]):
        font = load_font(name, allow_hinted=True)        # (DejaVuSans carries hinting instructions)
        for size in (16, 32):
            gs, places, runs, shape, jobs, jshape, lines = workload(font, args.lines, args.chars, size, seed=100 * fi + size)
            dgs = fr.DeviceGlyphSet(ctx, gs)
            plan = fr.TextPlan(dgs, places, runs, fr.FR_COVERAGE_U8, ns, fr.FR_SAMPLE_CENTER, fill)
            buf = torch.empty(shape, dtype=torch.uint8, device="cuda:0")
            torch.cuda.synchronize()
            ms = timed(plan, buf, shape, args.steps, args.warmup)
            px = plan.pixels
            desc = plan.describe()
            plan.close()
            del buf
            rgba = {}
            kinds = ([("rgba", 0)] if args.rgba or args.load else []) + ([("srgb", fr.FR_TEXT_SRGB)] if args.srgb or args.load else [])
            if kinds:
                words = [(225, 105, 180, 255), (40, 200, 90, 255)]
                cols = np.array([words[s[:k].count(" ") % 2] for s in lines for k in range(len(s))], np.uint8)
                clears = np.zeros((len(runs), 4), np.uint8)
                rbuf = torch.empty(shape + (4,), dtype=torch.uint8, device="cuda:0")
                if args.load:                          # the noise background, and the LOAD plans' own buffer
                    noise = torch.empty_like(rbuf).random_(0, 256, generator=torch.Generator("cuda:0").manual_seed(size))
                    lbuf = torch.empty_like(rbuf)
                for key, translucent in (("opaque", False), ("translucent", True)):
                    c = cols.copy()
                    if translucent:
                        c[:int(runs[0]["count"]), 3] = 160
                    for kind, flags in kinds:
                        rplan = fr.TextPlanRGBA(dgs, places, c, runs, clears, ns, fr.FR_SAMPLE_CENTER, flags | fill)
                        torch.cuda.synchronize()
                        # (with --load the clear-colour plans too render after a copy of the noise: the same cache state)
                        rms = (timed_over(rplan, rbuf, noise, shape, args.steps, args.warmup) if args.load
                               else timed(rplan, rbuf, shape, args.steps, args.warmup))
                        rgba[f"{kind}_{key}_ms"] = round(rms, 4)
                        rgba[f"{kind}_{key}_over_text"] = round(rms / ms, 3)
                        rgba[f"{kind}_{key}_plan"] = rplan.describe()
                        rplan.close()
                        if args.load:
                            lplan = fr.TextPlanRGBA(dgs, places, c, runs, None, ns, fr.FR_SAMPLE_CENTER, flags | fr.FR_TEXT_LOAD | fill)
                            torch.cuda.synchronize()
                            lms = timed_over(lplan, lbuf, noise, shape, args.steps, args.warmup)
                            rgba[f"{kind}_load_{key}_ms"] = round(lms, 4)
                            rgba[f"{kind}_load_{key}_over_{kind}"] = round(lms / rms, 3)
                            rgba[f"{kind}_load_{key}_plan"] = lplan.describe()
                            lplan.close()
                    if args.rgba and args.srgb:
                        rgba[f"srgb_{key}_over_rgba"] = round(rgba[f"srgb_{key}_ms"] / rgba[f"rgba_{key}_ms"], 3)
                del rbuf
                if args.load:
                    del noise, lbuf
            cells = fr.Plan(dgs, jobs, fr.FR_COVERAGE_U8, ns, fr.FR_SAMPLE_CENTER, fill)
            jbuf = torch.empty(jshape, dtype=torch.uint8, device="cuda:0")
            torch.cuda.synchronize()
            ms_cells = timed(cells, jbuf, jshape, args.steps, args.warmup)
            cpx, cdesc = cells.pixels, cells.describe()
            cells.close()
            del jbuf
            dgs.close()
            print(json.dumps({
                "font": name, "font_size": size, "lines": args.lines, "chars": args.chars, "samples": ns * ns,
                "instances": int(len(places)), "run_mpixel": round(px / 1e6, 3), "text_ms": round(ms, 4),
                "text_mpixel_per_s": round(px / 1e6 / (ms / 1e3), 1), "text_plan": desc,
                "cells_mpixel": round(cpx / 1e6, 3), "cells_ms": round(ms_cells, 4),
                "cells_mpixel_per_s": round(cpx / 1e6 / (ms_cells / 1e3), 1), "cells_plan": cdesc,
                "text_over_cells": round(ms / ms_cells, 2), **rgba}), flush=True)
    if args.load:
        overlay(ctx, args)
    ctx.close()


def place(ctx, args):
    """--place: (a) old plan, (b) _ex degenerate, (c) _ex slanted with random baseline fractions; coverage, RGBA opaque
    and RGBA translucent; alternated, --repeats times"""
    import torch
    ns, fill = args.samples, fr.FR_FILL_CONSISTENT if args.fill else 0
    med = lambda v: sorted(v)[len(v) // 2]
    for fi, name in enumerate(["DejaVuSans.ttf", "DejaVuSerif-Italic.ttf"]):
        font = load_font(name, allow_hinted=True)
        for size in (16, 32):
            gs, places, runs, shape, _, _, lines = workload(font, args.lines, args.chars, size, seed=100 * fi + size)
            rng = np.random.default_rng(size)
            degenerate = rg.make_places_ex([(int(p["glyph"]), int(p["pen_x64"]), 64 * int(p["pen_y"]), 0.0, 0.0) for p in places])
            slanted = degenerate.copy()
            slanted["pen_y64"] += rng.integers(0, 64, len(slanted)).astype(np.int32)
            slanted["slant"] = 0.2
            words = [(225, 105, 180, 255), (40, 200, 90, 255)]
            cols = np.array([words[s[:k].count(" ") % 2] for s in lines for k in range(len(s))], np.uint8)
            clears = np.zeros((len(runs), 4), np.uint8)
            dgs = fr.DeviceGlyphSet(ctx, gs)
            out = {"case": "place", "font": name, "font_size": size, "lines": args.lines, "chars": args.chars, "samples": ns * ns,
                   "instances": int(len(places)), "steps": args.steps, "repeats": args.repeats}
            for kind in ("text", "rgba_opaque", "rgba_translucent"):
                c = cols.copy()
                if kind == "rgba_translucent":
                    c[:int(runs[0]["count"]), 3] = 160
                make = ((lambda pl: fr.TextPlan(dgs, pl, runs, fr.FR_COVERAGE_U8, ns, fr.FR_SAMPLE_CENTER, fill)) if kind == "text" else
                        (lambda pl: fr.TextPlanRGBA(dgs, pl, c, runs, clears, ns, fr.FR_SAMPLE_CENTER, fill)))
                plans = {"a": make(places), "b": make(degenerate), "c": make(slanted)}
                bufs = {k: torch.zeros(shape + (() if kind == "text" else (4,)), dtype=torch.uint8, device="cuda:0") for k in plans}
                torch.cuda.synchronize()
                ms = {k: [] for k in plans}
                for _ in range(args.repeats):
                    for k, plan in plans.items():
                        ms[k].append(timed(plan, bufs[k], shape, args.steps, args.warmup))
                if not torch.equal(bufs["a"], bufs["b"]):
                    raise SystemExit(f"--place: {name} {size} {kind}: the degenerate _ex plan differs from the old plan")
                a, b, cc = med(ms["a"]), med(ms["b"]), med(ms["c"])
                out.update({f"{kind}_a_ms": round(a, 4), f"{kind}_a_min_ms": round(min(ms["a"]), 4), f"{kind}_a_max_ms": round(max(ms["a"]), 4),
                            f"{kind}_b_ms": round(b, 4), f"{kind}_c_ms": round(cc, 4), f"{kind}_b_over_a": round(b / a, 3),
                            f"{kind}_c_over_b": round(cc / b, 3), f"{kind}_a_plan": plans["a"].describe(),
                            f"{kind}_b_plan": plans["b"].describe()})
                for plan in plans.values():
                    plan.close()
                del bufs
            dgs.close()
            print(json.dumps(out), flush=True)


def cache(ctx, args):
    """--cache: (a) the plain coverage plan, (b) the same with FR_TEXT_CACHE; alternated, --repeats times; and the plain plan
    of every key placed once"""
    import re
    import torch
    ns, fill = args.samples, fr.FR_FILL_CONSISTENT if args.fill else 0
    med = lambda v: sorted(v)[len(v) // 2]
    for fi, name in enumerate(["DejaVuSans.ttf", "DejaVuSerif-Italic.ttf"]):
        font = load_font(name, allow_hinted=True)
        for size in (16, 32):
            gs, places, runs, shape, _, _, _ = workload(font, args.lines, args.chars, size, seed=100 * fi + size)
            scale = runs[0]["scale"]
            seg = gs.segments_per_glyph()
            # every key once, each in a run of its own as large as its cell, shelf-packed
            keys = sorted({(int(p["glyph"]), int(p["pen_x64"]) & 63) for p in places if seg[int(p["glyph"])]})
            kplaces, kruns, x, y, shelf, store = [], [], 0, 0, 0, 0
            for g, f in keys:
                c0, r0, cw, ch = fr.instance_cell(gs.boxes[g], scale, f, 0)
                store += 2 * cw * ch
                if x + cw > 16384:
                    x, y, shelf = 0, y + shelf, 0
                kruns.append((len(kplaces), 1, cw, ch, x, y, scale))
                kplaces.append((g, f - 64 * c0, -r0))
                x, shelf = x + cw, max(shelf, ch)
            kshape = (y + shelf, 16384)
            dgs = fr.DeviceGlyphSet(ctx, gs)
            make = lambda flags: fr.TextPlan(dgs, places, runs, fr.FR_COVERAGE_U8, ns, fr.FR_SAMPLE_CENTER, fill | flags)
            plans = {"a": make(0), "b": make(fr.FR_TEXT_CACHE)}
            bufs = {k: torch.zeros(shape, dtype=torch.uint8, device="cuda:0") for k in plans}
            torch.cuda.synchronize()
            ms = {k: [] for k in plans}
            for _ in range(args.repeats):
                for k, plan in plans.items():
                    ms[k].append(timed(plan, bufs[k], shape, args.steps, args.warmup))
            if not torch.equal(bufs["a"], bufs["b"]):
                raise SystemExit(f"--cache: {name} {size}: the cached plan differs from the plain plan")
            desc = plans["b"].describe()
            n_cells = int(re.search(r"glyph_mask_kernel<\d, \d> x(\d+)", desc).group(1))
            if n_cells != len(keys):
                raise SystemExit(f"--cache: {name} {size}: {n_cells} cells for {len(keys)} keys")
            kplan = fr.TextPlan(dgs, rg.make_places(kplaces), rg.make_runs(kruns), fr.FR_COVERAGE_U8, ns, fr.FR_SAMPLE_CENTER, fill)
            kbuf = torch.zeros(kshape, dtype=torch.uint8, device="cuda:0")
            torch.cuda.synchronize()
            kms = timed(kplan, kbuf, kshape, args.steps, args.warmup)
            a, b = med(ms["a"]), med(ms["b"])
            print(json.dumps({
                "case": "cache", "font": name, "font_size": size, "lines": args.lines, "chars": args.chars, "samples": ns * ns,
                "instances": int(re.search(r"text_cached_kernel<\d> x(\d+)", desc).group(1)), "cells": n_cells, "mask_store_bytes": store,
                "steps": args.steps, "repeats": args.repeats, "a_ms": round(a, 4), "a_min_ms": round(min(ms["a"]), 4),
                "a_max_ms": round(max(ms["a"]), 4), "b_ms": round(b, 4), "b_min_ms": round(min(ms["b"]), 4), "b_max_ms": round(max(ms["b"]), 4),
                "a_over_b": round(a / b, 2), "cells_only_ms": round(kms, 4), "b_minus_cells_only_ms": round(b - kms, 4),
                "a_plan": plans["a"].describe(), "b_plan": desc, "cells_only_plan": kplan.describe()}), flush=True)
            for plan in list(plans.values()) + [kplan]:
                plan.close()
            del bufs, kbuf
            dgs.close()


def over(ctx, args):
    """--over: the --rgba translucent colouring as (a) the plan without FR_TEXT_OVER, (b) the plan with it; UNORM and sRGB;
    alternated, --repeats times"""
    import torch
    ns, fill = args.samples, fr.FR_FILL_CONSISTENT if args.fill else 0
    med = lambda v: sorted(v)[len(v) // 2]
    for fi, name in enumerate(["DejaVuSans.ttf", "DejaVuSerif-Italic.ttf"]):
        font = load_font(name, allow_hinted=True)
        for size in (16, 32):
            gs, places, runs, shape, _, _, lines = workload(font, args.lines, args.chars, size, seed=100 * fi + size)
            words = [(225, 105, 180, 255), (40, 200, 90, 255)]
            cols = np.array([words[s[:k].count(" ") % 2] for s in lines for k in range(len(s))], np.uint8)
            cols[:int(runs[0]["count"]), 3] = 160
            clears = np.zeros((len(runs), 4), np.uint8)
            dgs = fr.DeviceGlyphSet(ctx, gs)
            out = {"case": "over", "font": name, "font_size": size, "lines": args.lines, "chars": args.chars, "samples": ns * ns,
                   "instances": int(len(places)), "steps": args.steps, "repeats": args.repeats}
            for kind, space in (("rgba", 0), ("srgb", fr.FR_TEXT_SRGB)):
                make = lambda flags: fr.TextPlanRGBA(dgs, places, cols, runs, clears, ns, fr.FR_SAMPLE_CENTER, space | fill | flags)
                plans = {"a": make(0), "b": make(fr.FR_TEXT_OVER)}
                bufs = {k: torch.zeros(shape + (4,), dtype=torch.uint8, device="cuda:0") for k in plans}
                torch.cuda.synchronize()
                ms = {k: [] for k in plans}
                for _ in range(args.repeats):
                    for k, plan in plans.items():
                        ms[k].append(timed(plan, bufs[k], shape, args.steps, args.warmup))
                if not torch.equal(bufs["a"][..., :3], bufs["b"][..., :3]):
                    raise SystemExit(f"--over: {name} {size} {kind}: R G B differ from the plan without the flag")
                a, b = med(ms["a"]), med(ms["b"])
                out.update({f"{kind}_a_ms": round(a, 4), f"{kind}_a_min_ms": round(min(ms["a"]), 4), f"{kind}_a_max_ms": round(max(ms["a"]), 4),
                            f"{kind}_b_ms": round(b, 4), f"{kind}_b_min_ms": round(min(ms["b"]), 4), f"{kind}_b_max_ms": round(max(ms["b"]), 4),
                            f"{kind}_b_over_a": round(b / a, 3), f"{kind}_a_plan": plans["a"].describe(), f"{kind}_b_plan": plans["b"].describe()})
                for plan in plans.values():
                    plan.close()
                del bufs
            dgs.close()
            print(json.dumps(out), flush=True)


def rotated_runs(gs, places, runs, scale, angle_deg, width=16384):
    """the workload's lines turned by angle_deg about each line's pen origin, as fr_glyph_place_affine placements with
    m = scale * R(angle): every line in a run of its own that is the union of its instance cells (include/fr_raster.h),
    the runs shelf-packed into an image at most `width` columns wide -> (places, runs, shape)"""
    import math
    f = np.float32
    c, sn = {0: (1.0, 0.0), 90: (0.0, 1.0)}.get(angle_deg, (math.cos(math.radians(angle_deg)), math.sin(math.radians(angle_deg))))
    s = float(scale)
    m = np.array([s * c, -s * sn, s * sn, s * c]).astype(f)
    out = np.zeros(len(places), rg.PLACE_AFFINE_DTYPE)
    out["glyph"], out["m"] = places["glyph"], m
    first = runs["first"].astype(np.int64)
    pen0 = np.repeat(places["pen_x64"][first], runs["count"].astype(np.int64))
    p = (places["pen_x64"] - pen0).astype(np.float64)                        # along the baseline, 1/64 pixel
    px, py = np.floor(c * p + 0.5).astype(np.int64), np.floor(-sn * p + 0.5).astype(np.int64)
    box = gs.boxes[places["glyph"]].astype(f)
    xs, ys = box[:, [0, 0, 2, 2]], box[:, [1, 3, 1, 3]]
    u = (m[0] * xs).astype(f) + (m[1] * ys).astype(f)
    v = (m[2] * xs).astype(f) + (m[3] * ys).astype(f)
    mnx, mxx = np.floor(u.min(1)).astype(np.int64), np.ceil(u.max(1)).astype(np.int64)
    mny, mxy = np.floor(v.min(1)).astype(np.int64), np.ceil(v.max(1)).astype(np.int64)
    x0, y0 = (px >> 6) + mnx, (py >> 6) - mxy
    x1, y1 = x0 + (mxx - mnx + 1 + ((px & 63) != 0)), y0 + (mxy - mny + 1 + ((py & 63) != 0))
    left, top = np.minimum.reduceat(x0, first), np.minimum.reduceat(y0, first)
    w, h = np.maximum.reduceat(x1, first) - left, np.maximum.reduceat(y1, first) - top
    cnt = runs["count"].astype(np.int64)
    out["pen_x64"], out["pen_y64"] = px - 64 * np.repeat(left, cnt), py - 64 * np.repeat(top, cnt)
    rows, x, y, shelf = [], 0, 0, 0
    for r in range(len(runs)):
        if x + int(w[r]) > width:
            x, y, shelf = 0, y + shelf, 0
        rows.append((int(first[r]), int(cnt[r]), int(w[r]), int(h[r]), x, y, 1.0))
        x, shelf = x + int(w[r]), max(shelf, int(h[r]))
    return out, rg.make_runs(rows), (y + shelf, min(width, max(int(w.max()), max(r[4] + r[2] for r in rows))))


def affine(ctx, args):
    """--affine: (a) the _ex plan, (b)-(e) the affine plan at 0, 5, 45 and 90 degrees; coverage; alternated, --repeats times"""
    import torch
    ns, fill = args.samples, fr.FR_FILL_CONSISTENT if args.fill else 0
    med = lambda v: sorted(v)[len(v) // 2]
    for fi, name in enumerate(["DejaVuSans.ttf", "DejaVuSerif-Italic.ttf"]):
        font = load_font(name, allow_hinted=True)
        for size in (16, 32):
            gs, places, runs, shape, _, _, _ = workload(font, args.lines, args.chars, size, seed=100 * fi + size)
            ex = rg.make_places_ex([(int(p["glyph"]), int(p["pen_x64"]), 64 * int(p["pen_y"]), 0.0, 0.0) for p in places])
            dgs = fr.DeviceGlyphSet(ctx, gs)
            forms = {"a": (ex, runs, shape)}
            for key, angle in (("b", 0), ("c", 5), ("d", 45), ("e", 90)):
                forms[key] = rotated_runs(gs, places, runs, runs[0]["scale"], angle)
            plans = {k: fr.TextPlan(dgs, pl, rn, fr.FR_COVERAGE_U8, ns, fr.FR_SAMPLE_CENTER, fill) for k, (pl, rn, _) in forms.items()}
            bufs = {k: torch.zeros(sh, dtype=torch.uint8, device="cuda:0") for k, (_, _, sh) in forms.items()}
            torch.cuda.synchronize()
            ms = {k: [] for k in plans}
            for _ in range(args.repeats):
                for k, plan in plans.items():
                    ms[k].append(timed(plan, bufs[k], forms[k][2], args.steps, args.warmup))
            out = {"case": "affine", "font": name, "font_size": size, "lines": args.lines, "chars": args.chars, "samples": ns * ns,
                   "instances": int(len(places)), "steps": args.steps, "repeats": args.repeats}
            a = med(ms["a"])
            for k, plan in plans.items():
                out.update({f"{k}_ms": round(med(ms[k]), 4), f"{k}_min_ms": round(min(ms[k]), 4), f"{k}_max_ms": round(max(ms[k]), 4),
                            f"{k}_run_mpixel": round(plan.pixels / 1e6, 1), f"{k}_lit_fraction": round(int(torch.count_nonzero(bufs[k])) / bufs[k].numel(), 4)})
                if k != "a":
                    out[f"{k}_over_a"] = round(med(ms[k]) / a, 2)
            out.update({"a_plan": plans["a"].describe(), "e_plan": plans["e"].describe()})
            for plan in plans.values():
                plan.close()
            del bufs
            dgs.close()
            print(json.dumps(out), flush=True)


def affine_store(gs, pl):
    """-> (keys, bytes of the mask store) of the FR_TEXT_CACHE_AFFINE plan of rotated_runs' placements, all under one matrix
    and none clipped: one cell per (glyph, both pen fractions), 2 bytes per element (include/fr_raster.h)"""
    f = np.float32
    m = pl["m"][0]
    box = gs.boxes[pl["glyph"]].astype(f)
    xs, ys = box[:, [0, 0, 2, 2]], box[:, [1, 3, 1, 3]]
    u = (m[0] * xs).astype(f) + (m[1] * ys).astype(f)
    v = (m[2] * xs).astype(f) + (m[3] * ys).astype(f)
    fx, fy = pl["pen_x64"].astype(np.int64) & 63, pl["pen_y64"].astype(np.int64) & 63
    cw = np.ceil(u.max(1)).astype(np.int64) - np.floor(u.min(1)).astype(np.int64) + 1 + (fx != 0)
    ch = np.ceil(v.max(1)).astype(np.int64) - np.floor(v.min(1)).astype(np.int64) + 1 + (fy != 0)
    drawn = gs.segments_per_glyph()[pl["glyph"]] > 0
    keys = np.stack([pl["glyph"].astype(np.int64), fx, fy], 1)[drawn]
    _, first = np.unique(keys, axis=0, return_index=True)
    return len(first), int(2 * (cw[drawn][first] * ch[drawn][first]).sum())


def affine_cache(ctx, args):
    """--affine --cache: the five variants of --affine, each as the plain and as the cached plan; alternated, --repeats times"""
    import re
    import torch
    ns, fill = args.samples, fr.FR_FILL_CONSISTENT if args.fill else 0
    med = lambda v: sorted(v)[len(v) // 2]
    for fi, name in enumerate(["DejaVuSans.ttf", "DejaVuSerif-Italic.ttf"]):
        font = load_font(name, allow_hinted=True)
        for size in (16, 32):
            gs, places, runs, shape, _, _, _ = workload(font, args.lines, args.chars, size, seed=100 * fi + size)
            ex = rg.make_places_ex([(int(p["glyph"]), int(p["pen_x64"]), 64 * int(p["pen_y"]), 0.0, 0.0) for p in places])
            dgs = fr.DeviceGlyphSet(ctx, gs)
            forms = {"a": (ex, runs, shape)}
            for key, angle in (("b", 0), ("c", 5), ("d", 45), ("e", 90)):
                forms[key] = rotated_runs(gs, places, runs, runs[0]["scale"], angle)
            seg = gs.segments_per_glyph()
            ekeys = sorted({(int(p["glyph"]), int(p["pen_x64"]) & 63) for p in places if seg[int(p["glyph"])]})
            store = {"a": (len(ekeys), sum(2 * cw * ch for _, _, cw, ch in (fr.instance_cell(gs.boxes[g], runs[0]["scale"], fx, 0) for g, fx in ekeys)))}
            store.update({k: affine_store(gs, forms[k][0]) for k in "bcde"})
            plans, bufs = {}, {}
            for k, (pl, rn, sh) in forms.items():
                for c, flag in (("", 0), ("_cached", fr.FR_TEXT_CACHE if k == "a" else fr.FR_TEXT_CACHE_AFFINE)):
                    plans[k + c] = fr.TextPlan(dgs, pl, rn, fr.FR_COVERAGE_U8, ns, fr.FR_SAMPLE_CENTER, fill | flag)
                    bufs[k + c] = torch.zeros(sh, dtype=torch.uint8, device="cuda:0")
            torch.cuda.synchronize()
            ms = {k: [] for k in plans}
            for _ in range(args.repeats):
                for k, plan in plans.items():
                    ms[k].append(timed(plan, bufs[k], forms[k[0]][2], args.steps, args.warmup))
            out = {"case": "affine_cache", "font": name, "font_size": size, "lines": args.lines, "chars": args.chars, "samples": ns * ns,
                   "steps": args.steps, "repeats": args.repeats}
            for k in forms:
                if not torch.equal(bufs[k], bufs[k + "_cached"]):
                    raise SystemExit(f"--affine --cache: {name} {size} ({k}): the cached plan differs from the plain plan")
                desc = plans[k + "_cached"].describe()
                n_cells = int(re.search(r"glyph_mask(?:_affine)?_kernel<\d, \d> x(\d+)", desc).group(1))
                if n_cells != store[k][0]:
                    raise SystemExit(f"--affine --cache: {name} {size} ({k}): {n_cells} cells for {store[k][0]} keys")
                out.update({f"{k}_instances": int(re.search(r"text_cached_kernel<\d> x(\d+)", desc).group(1)), f"{k}_cells": n_cells,
                            f"{k}_mask_store_bytes": store[k][1], f"{k}_run_mpixel": round(plans[k].pixels / 1e6, 1)})
                for c in ("", "_cached"):
                    v = ms[k + c]
                    out.update({f"{k}{c}_ms": round(med(v), 4), f"{k}{c}_min_ms": round(min(v), 4), f"{k}{c}_max_ms": round(max(v), 4)})
                out[f"{k}_plain_over_cached"] = round(med(ms[k]) / med(ms[k + "_cached"]), 2)
            out.update({"a_cached_plan": plans["a_cached"].describe(), "e_cached_plan": plans["e_cached"].describe()})
            for plan in plans.values():
                plan.close()
            del bufs
            dgs.close()
            print(json.dumps(out), flush=True)


def tiles_met(places, run, gs, scale):
    """the 64 x 16 tiles of `run` that some clipped instance cell meets (what a LOAD plan launches)"""
    w, h, seg, met = int(run["w"]), int(run["h"]), gs.segments_per_glyph(), set()
    for pl in places[int(run["first"]):int(run["first"]) + int(run["count"])]:
        if not seg[int(pl["glyph"])]:
            continue
        c0, r0, cw, ch = fr.instance_cell(gs.boxes[int(pl["glyph"])], scale, int(pl["pen_x64"]), int(pl["pen_y"]))
        x0, x1, y0, y1 = max(c0, 0), min(c0 + cw, w), max(r0, 0), min(r0 + ch, h)
        if x0 < x1 and y0 < y1:
            met |= {(ty, tx) for ty in range(y0 // 16, (y1 - 1) // 16 + 1) for tx in range(x0 // 64, (x1 - 1) // 64 + 1)}
    return len(met)


def overlay(ctx, args):
    """(b): 16 lines of 64 characters, size 32, on a 3840 x 2160 frame: one LOAD run over the frame vs one clear-colour run"""
    import torch
    ns, fill = args.samples, fr.FR_FILL_CONSISTENT if args.fill else 0
    W, H, size, n_lines, n_chars = 3840, 2160, 32, 16, 64
    font = load_font("DejaVuSans.ttf", allow_hinted=True)
    rng = np.random.default_rng(7)
    alphabet = [chr(c) for c in range(0x20, 0x7f)]
    lay = [font.layout("".join(rng.choice(alphabet, n_chars)), size) for _ in range(n_lines)]
    gs, kept = font.glyphset(sorted({int(g) for gi, _, _ in lay for g in gi}), skip_unsupported=False)
    local = {g: k for k, g in enumerate(kept)}
    scale = np.float32(size) / np.float32(font.information.units_per_em)
    places = rg.make_places([(local[int(g)], 64 * 160 + 21 + int(p), 120 + 128 * i)
                             for i, (gi, pen, _) in enumerate(lay) for g, p in zip(gi, pen)])
    runs = rg.make_runs([(0, len(places), W, H, 0, 0, scale)])
    cols = np.array([(255, 255, 255, 255)] * len(places), np.uint8)
    dgs = fr.DeviceGlyphSet(ctx, gs)
    noise = torch.empty((H, W, 4), dtype=torch.uint8, device="cuda:0").random_(0, 256, generator=torch.Generator("cuda:0").manual_seed(1))
    cbuf, lbuf = torch.empty_like(noise), torch.empty_like(noise)     # the clear-colour plans' output; the LOAD plans'
    out = {"case": "overlay", "frame": [W, H], "lines": n_lines, "chars": n_chars, "font_size": size,
           "instances": int(len(places)), "tiles_clear": ((W + 63) // 64) * ((H + 15) // 16),
           "tiles_load_computed": tiles_met(places, runs[0], gs, scale)}
    for key, alpha in (("opaque", 255), ("translucent", 200)):
        cols[:, 3] = alpha
        for kind, flags in (("rgba", 0), ("srgb", fr.FR_TEXT_SRGB)):
            for load in (False, True):
                plan = fr.TextPlanRGBA(dgs, places, cols, runs, None if load else [(0, 0, 0, 0)], ns, fr.FR_SAMPLE_CENTER,
                                       flags | (fr.FR_TEXT_LOAD if load else 0) | fill)
                torch.cuda.synchronize()
                tag = f"{kind}{'_load' if load else ''}_{key}"
                ms = timed_over(plan, lbuf if load else cbuf, noise, (H, W), args.steps, args.warmup)
                out[tag + "_ms"] = round(ms, 4)
                out[tag + "_plan"] = plan.describe()
                plan.close()
            out[f"{kind}_{key}_clear_over_load"] = round(out[f"{kind}_{key}_ms"] / out[f"{kind}_load_{key}_ms"], 3)
    del noise, cbuf, lbuf
    dgs.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()

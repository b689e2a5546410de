"""Sub-pixel text benchmark: fr_layer_lcd, the tile kernel of csrc/fr_layer_lcd.hip, against the
one-colour route a caller had before it.  Everything runs in one process, the alternatives alternated --repeats times; every
figure is the median over the repeats, with the smallest and largest repeat beside it.  "ms" is device time per call: HIP
events on the context's stream around --calls back-to-back calls, so it holds the table upload of each call and any gap the
host leaves.  Prints one JSON line per configuration.

Case "frame": fr_layer_lcd of a text-like plane of 3 x 3840 x 2160 elements (tools/bench_layer.py's frame of lines, rendered
three times as wide through the affine text plan) onto a noise frame, UNORM and sRGB, against fr_layer_paint with one stop
through the 4-byte layer of the same lines.  "bytes_per_px" is the kernel's traffic model by its skip rules per lane group
of four pixels: 3 (the plane read alone) where the group's sixteen plane bytes are all zero, 3 + 4 where they are all 255
(the store), else 3 + 8 (load and store); for fr_layer_paint 4 / 8 / 12 likewise.  "tb_per_s" is that traffic over the time,
"share_of_8TBs" the same over 8 TB/s.

Case "lines": the 4 096 lines of tools/bench_text.py as the whole route per frame: the affine 3x coverage plan's render plus
fr_layer_lcd, against the _ex RGBA plan's render (FR_TEXT_OVER over a clear layer) plus fr_layer_paint with one stop.
--cache adds the same 3x plan with FR_TEXT_CACHE_AFFINE (one mask cell per (glyph, pen fraction) of the plane, filled once
per render: csrc/fr_text_cached.hip) as routes of its own, alternated with the others; the two planes must be equal, and
the summary line states the instances, the cells and the bytes of the mask store.

    python tools/bench_lcd.py [--calls 50] [--repeats 5] [--lines 4096] [--cases frame,lines] [--cache]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]

import font_renderer_amd as fr  # noqa: E402
from bench_layer import bytes_per_px, stats, time_calls  # noqa: E402
from bench_text import workload  # noqa: E402
from fixtures import load_font  # noqa: E402

COLOUR = (20, 10, 0, 255)


def report(case, route, res, px, bpp, **extra):
    ms, lo, hi = stats([r[0] for r in res[1:]])                          # the first round warms up
    line = {"case": case, "route": route, **extra, "ms": round(ms, 4), "min_ms": round(lo, 4), "max_ms": round(hi, 4),
            "host_ms": round(stats([r[1] for r in res[1:]])[0], 4)}
    if bpp is not None:
        line.update({"bytes_per_px": round(bpp, 2), "tb_per_s": round(px * bpp / (ms * 1e-3) / 1e12, 3), "share_of_8TBs": round(px * bpp / (ms * 1e-3) / 8e12, 3)})
    print(json.dumps(line), flush=True)
    return ms


def lcd_bytes_per_px(plane):
    """the kernel's traffic per pixel for `plane` ((rows, 3 w) u8 on the host, w a multiple of 4, one window over all of it)
    at A = 255 with the default filter: per lane group the twelve elements and the two taps on either side"""
    rows, n = plane.shape
    pad = np.zeros((rows, n + 4), np.uint8)
    pad[:, 2:-2] = plane
    g = n // 12
    core = pad[:, 2:-2].reshape(rows, g, 12)
    left = pad[:, :n].reshape(rows, g, 12)[..., :2]
    right = pad[:, 4:].reshape(rows, g, 12)[..., -2:]
    zero = ~(core.any(-1) | left.any(-1) | right.any(-1))
    full = (core == 255).all(-1) & (left == 255).all(-1) & (right == 255).all(-1)
    return float(np.where(zero, 3, np.where(full, 7, 11)).mean())


def as_lcd(places, runs):
    """fr_glyph_place rows and their runs three times as wide: m = {3 s, 0, 0, s}, the pens' x tripled"""
    rows = []
    for r in runs:
        s = float(r["scale"])
        for k in range(int(r["first"]), int(r["first"]) + int(r["count"])):
            p = places[k]
            rows.append((int(p["glyph"]), 3 * int(p["pen_x64"]), 64 * int(p["pen_y"]), 3.0 * s, 0.0, 0.0, s))
    wide = runs.copy()
    wide["w"] *= 3
    wide["out_x"] *= 3
    return fr.make_places_affine(rows), wide


def as_ex(places, runs):
    return fr.make_places_ex([(int(p["glyph"]), int(p["pen_x64"]), 64 * int(p["pen_y"]), 0.0, 0.0) for p in places])


def noise_frame(H, W):
    import torch
    frame = torch.empty((H, W, 4), dtype=torch.uint8, device="cuda:0").random_(0, 256, generator=torch.Generator("cuda:0").manual_seed(W))
    frame[..., 3] = 255
    return frame


def mask_store_bytes(gs, wide_places):
    """-> (keys, bytes of the mask store) of the FR_TEXT_CACHE_AFFINE plan of these placements: one cell per (glyph, both pen
    fractions) under the one matrix, 2 bytes per element (include/fr_raster.h)"""
    seg = gs.segments_per_glyph()
    keys = sorted({(int(p["glyph"]), int(p["pen_x64"]) & 63, int(p["pen_y64"]) & 63) for p in wide_places if seg[int(p["glyph"])]})
    m = wide_places["m"][0]
    return len(keys), sum(2 * int(cw) * int(ch) for _, _, cw, ch in (fr.instance_cell_affine(gs.boxes[g], m, fx, fy) for g, fx, fy in keys))


def routes_of(ctx, gs, places, runs, shape, samples=4):
    """the two renders of the lines, into buffers of shape = (H, W): -> (dgs, lcd plan, plane, ex plan, layer)"""
    import torch
    H, W = shape
    dgs = fr.DeviceGlyphSet(ctx, gs)
    wide_places, wide_runs = as_lcd(places, runs)
    lcd_plan = fr.TextPlan(dgs, wide_places, wide_runs, fr.FR_COVERAGE_U8, samples, fr.FR_SAMPLE_CENTER, fr.FR_FILL_CONSISTENT)
    cols = np.tile(np.array([255, 255, 255, 255], np.uint8), (len(places), 1))
    ex_plan = fr.TextPlanRGBA(dgs, as_ex(places, runs), cols, runs, np.zeros((len(runs), 4), np.uint8), samples, fr.FR_SAMPLE_CENTER,
                              fr.FR_FILL_CONSISTENT | fr.FR_TEXT_OVER)
    plane = torch.zeros((H, 3 * W), dtype=torch.uint8, device="cuda:0")
    layer = torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    lcd_plan.render(plane.data_ptr(), 3 * W, H)
    ex_plan.render(layer.data_ptr(), W, H)
    ctx.sync()
    return dgs, lcd_plan, plane, ex_plan, layer


def frame_case(ctx, stream, args, font):
    W, H = 3840, 2160
    gs, places, runs, shape, _, _, _ = workload(font, H // 19, W // 10, 16, seed=5)
    import torch
    dgs, lcd_plan, whole_plane, ex_plan, whole_layer = routes_of(ctx, gs, places, runs, tuple(shape))
    lcd_plan.close(), ex_plan.close(), dgs.close()
    # the frame's part of the lines' own size, as tools/bench_layer.py cuts it
    h, w = min(H, shape[0]), min(W, shape[1])
    plane = torch.zeros((H, 3 * W), dtype=torch.uint8, device="cuda:0")
    layer = torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda:0")
    plane[:h, :3 * w] = whole_plane[:h, :3 * w]
    layer[:h, :w] = whole_layer[:h, :w]
    del whole_plane, whole_layer
    torch.cuda.synchronize()
    frame = noise_frame(H, W)
    blits = fr.make_lcd_blits([(0, 0, W, H, 0, 0, COLOUR)])
    one = fr.make_gradient_linear(0, 0, 64 * W, 0, [(0, COLOUR)])
    lcd_bpp, paint_bpp = lcd_bytes_per_px(plane.cpu().numpy()), bytes_per_px(layer.cpu().numpy(), 255)
    routes = {}
    for srgb in (False, True):
        routes[("lcd", srgb)] = (lambda k, srgb=srgb: fr.layer_lcd(ctx, plane.data_ptr(), 3 * W, H, frame.data_ptr(), W, H, blits, None, srgb), lcd_bpp)
        routes[("paint", srgb)] = (lambda k, srgb=srgb: fr.layer_paint(ctx, layer.data_ptr(), W, H, frame.data_ptr(), W, H, one, (0, 0, W, H), (0, 0), srgb), paint_bpp)
    res = {r: [] for r in routes}
    for _ in range(args.repeats + 1):
        for r, (fn, _) in routes.items():
            res[r].append(time_calls(ctx, stream, args.calls, fn))
    ms = {r: report("frame", r[0], res[r], W * H, routes[r][1], w=W, h=H, srgb=r[1]) for r in routes}
    for srgb in (False, True):
        print(json.dumps({"case": "frame", "srgb": srgb, "lcd_ms_by_paint_ms": round(ms[("lcd", srgb)] / ms[("paint", srgb)], 3)}), flush=True)


def lines_case(ctx, stream, args, font):
    gs, places, runs, shape, _, _, _ = workload(font, args.lines, 64, 16, seed=16)
    H, W = shape[0], (shape[1] + 3) // 4 * 4
    dgs, lcd_plan, plane, ex_plan, layer = routes_of(ctx, gs, places, runs, (H, W))
    frame = noise_frame(H, W)
    blits = fr.make_lcd_blits([(0, 0, W, H, 0, 0, COLOUR)])
    one = fr.make_gradient_linear(0, 0, 64 * W, 0, [(0, COLOUR)])

    def lcd(k):
        lcd_plan.render(plane.data_ptr(), 3 * W, H)
        fr.layer_lcd(ctx, plane.data_ptr(), 3 * W, H, frame.data_ptr(), W, H, blits)

    def paint(k):
        ex_plan.render(layer.data_ptr(), W, H)
        fr.layer_paint(ctx, layer.data_ptr(), W, H, frame.data_ptr(), W, H, one, (0, 0, W, H), (0, 0))

    routes = {"affine3x+lcd": lcd, "ex_rgba+paint": paint,
              "affine3x_render": lambda k: lcd_plan.render(plane.data_ptr(), 3 * W, H), "ex_rgba_render": lambda k: ex_plan.render(layer.data_ptr(), W, H)}
    if args.cache:
        import re
        import torch
        wide_places, wide_runs = as_lcd(places, runs)
        cached_plan = fr.TextPlan(dgs, wide_places, wide_runs, fr.FR_COVERAGE_U8, 4, fr.FR_SAMPLE_CENTER, fr.FR_FILL_CONSISTENT | fr.FR_TEXT_CACHE_AFFINE)
        cached_plane = torch.zeros_like(plane)
        torch.cuda.synchronize()

        def cached(k):
            cached_plan.render(cached_plane.data_ptr(), 3 * W, H)
            fr.layer_lcd(ctx, cached_plane.data_ptr(), 3 * W, H, frame.data_ptr(), W, H, blits)

        routes.update({"affine3x_cached+lcd": cached, "affine3x_cached_render": lambda k: cached_plan.render(cached_plane.data_ptr(), 3 * W, H)})
    res = {r: [] for r in routes}
    for _ in range(args.repeats + 1):
        for r, fn in routes.items():
            res[r].append(time_calls(ctx, stream, args.calls, fn))
    ms = {r: report("lines", r, res[r], W * H, None, lines=args.lines, w=W, h=H) for r in routes}
    print(json.dumps({"case": "lines", "lcd_route_ms_by_paint_route_ms": round(ms["affine3x+lcd"] / ms["ex_rgba+paint"], 3),
                      "render_share_of_lcd_route": round(ms["affine3x_render"] / ms["affine3x+lcd"], 3)}), flush=True)
    if args.cache:
        ctx.sync()
        if not torch.equal(plane, cached_plane):
            raise SystemExit("--cache: the cached 3x plan's plane differs from the plain plan's")
        desc = cached_plan.describe()
        n_keys, store = mask_store_bytes(gs, wide_places)
        n_cells = int(re.search(r"glyph_mask_affine_kernel<\d, \d> x(\d+)", desc).group(1))
        if n_cells != n_keys:
            raise SystemExit(f"--cache: {n_cells} cells for {n_keys} keys")
        print(json.dumps({"case": "lines", "cache": True, "instances": int(re.search(r"text_cached_kernel<\d> x(\d+)", desc).group(1)), "cells": n_cells,
                          "mask_store_bytes": store, "plain_render_by_cached_render": round(ms["affine3x_render"] / ms["affine3x_cached_render"], 2),
                          "plain_route_by_cached_route": round(ms["affine3x+lcd"] / ms["affine3x_cached+lcd"], 2),
                          "cached_route_ms_by_paint_route_ms": round(ms["affine3x_cached+lcd"] / ms["ex_rgba+paint"], 3),
                          "render_share_of_cached_route": round(ms["affine3x_cached_render"] / ms["affine3x_cached+lcd"], 3), "cached_plan": desc}), flush=True)
        cached_plan.close()
    lcd_plan.close(), ex_plan.close(), dgs.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50, help="calls per timing")
    ap.add_argument("--repeats", type=int, default=5, help="repeats of each alternated timing")
    ap.add_argument("--lines", type=int, default=4096)
    ap.add_argument("--cases", default="frame,lines", help="which of frame and lines to run")
    ap.add_argument("--cache", action="store_true", help="lines: also the 3x plan with FR_TEXT_CACHE_AFFINE, alternated with the plain one")
    args = ap.parse_args()
    import torch
    stream = torch.cuda.Stream(device="cuda:0")
    ctx = fr.Context(0, stream.cuda_stream)
    font = load_font("DejaVuSans.ttf", allow_hinted=True)
    cases = args.cases.split(",")
    if "frame" in cases:
        frame_case(ctx, stream, args, font)
    if "lines" in cases:
        lines_case(ctx, stream, args, font)
    ctx.close()


if __name__ == "__main__":
    main()

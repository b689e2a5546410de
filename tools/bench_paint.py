"""Gradient benchmark: fr_layer_paint, the tile kernel of csrc/fr_layer_paint.hip, against the
routes a caller had before it.  Everything runs in one process, the alternatives alternated --repeats times; every figure
is the median over the repeats, with the smallest and largest repeat beside it.  "ms" is device time per call: HIP events
on the context's stream around --calls back-to-back calls, so it holds the table upload of each call and any gap the host
leaves.  Prints one JSON line per configuration.

Case "text": a two-stop linear and a two-stop radial gradient through a text layer over a noise frame, against the flat
colour a caller had: fr_layer_shadow without a stage (the layer's alpha tinted into a second layer) plus fr_layer_over of
that layer.  Two layers: the text-like 3840 x 2160 layer of tools/bench_layer.py's frame case, and its 4 096 lines of 64
characters at size 16 as one layer of their own size.  "bytes_per_px" is the kernel's traffic model by its skip rules
per lane group of four pixels: 4 (the layer read alone) where every a is 0, 8 where every a is 255 (the store), else 12
(load and store); for the other route 8 per pixel of the tint plus fr_layer_over's 4 / 8 / 12.  "tb_per_s" is that traffic
over the time, "share_of_8TBs" the same over 8 TB/s.

Case "panel": full coverage (no layer), opaque stops, over a whole 3840 x 2160 and 7680 x 4320 frame: 4 bytes per pixel,
against fr_layer_rects with one opaque rectangle of the frame's size (4 bytes per pixel too).

    python tools/bench_paint.py [--calls 50] [--repeats 5] [--lines 4096] [--cases text,panel,big]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]

import font_renderer_amd as fr  # noqa: E402
from bench_layer import bytes_per_px, render_layer, stats, time_calls  # noqa: E402
from bench_text import workload  # noqa: E402
from fixtures import load_font  # noqa: E402

STOPS = [(0, (255, 90, 0, 255)), (65536, (0, 120, 255, 255))]


def report(case, route, res, px, bpp, **extra):
    ms, lo, hi = stats([r[0] for r in res[1:]])                          # the first round warms up
    print(json.dumps({"case": case, "route": route, **extra, "ms": round(ms, 4), "min_ms": round(lo, 4), "max_ms": round(hi, 4),
                      "host_ms": round(stats([r[1] for r in res[1:]])[0], 4), "bytes_per_px": round(bpp, 2),
                      "tb_per_s": round(px * bpp / (ms * 1e-3) / 1e12, 3), "share_of_8TBs": round(px * bpp / (ms * 1e-3) / 8e12, 3)}), flush=True)
    return ms


def gradients(W, H):
    return {"linear": fr.make_gradient_linear(0, 0, 64 * W, 64 * H, STOPS), "radial": fr.make_gradient_radial(32 * W, 32 * H, 32 * min(W, H), STOPS, fr.FR_SPREAD_REFLECT)}


def text_case(ctx, stream, args, name, layer):
    """layer: (H, W, 4) premultiplied on the device, W a multiple of 4"""
    import torch
    H, W = layer.shape[:2]
    frame = torch.empty((H, W, 4), dtype=torch.uint8, device="cuda:0").random_(0, 256, generator=torch.Generator("cuda:0").manual_seed(W))
    frame[..., 3] = 255
    tinted = torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    blit = fr.make_blits([(0, 0, W, H, 0, 0, 255)])
    host = layer.cpu().numpy()
    bpp = bytes_per_px(host, 255)                               # opaque stops: a = cov, so fr_layer_over's groups are this kernel's
    routes = {}
    for srgb in (False, True):
        for kind, g in gradients(W, H).items():
            routes[(kind, srgb)] = (lambda k, g=g, srgb=srgb: fr.layer_paint(ctx, layer.data_ptr(), W, H, frame.data_ptr(), W, H, g, (0, 0, W, H), (0, 0), srgb), bpp)

        def flat(k, srgb=srgb):
            fr.layer_shadow(ctx, layer.data_ptr(), W, H, tinted.data_ptr(), W, H, (0, 0, W, H), (0, 0, W, H), (0, 0), 0, 0, 0, STOPS[0][1], srgb)
            fr.layer_over(ctx, tinted.data_ptr(), W, H, frame.data_ptr(), W, H, blit, srgb)
        routes[("shadow+over", srgb)] = (flat, 8 + bpp)
    res = {r: [] for r in routes}
    for _ in range(args.repeats + 1):
        for r, (fn, _) in routes.items():
            res[r].append(time_calls(ctx, stream, args.calls, fn))
    ms = {r: report("text", r[0], res[r], W * H, routes[r][1], layer=name, w=W, h=H, srgb=r[1]) for r in routes}
    for srgb in (False, True):
        print(json.dumps({"case": "text", "layer": name, "srgb": srgb, "shadow_over_ms_by_linear_ms": round(ms[("shadow+over", srgb)] / ms[("linear", srgb)], 3),
                          "radial_ms_by_linear_ms": round(ms[("radial", srgb)] / ms[("linear", srgb)], 3)}), flush=True)


def panel_case(ctx, stream, args, W, H):
    import torch
    frame = torch.empty((H, W, 4), dtype=torch.uint8, device="cuda:0").random_(0, 256, generator=torch.Generator("cuda:0").manual_seed(W))
    frame[..., 3] = 255
    torch.cuda.synchronize()
    rect = fr.make_rects([(0, 0, 64 * W, 64 * H, STOPS[0][1])])
    routes = {}
    for srgb in (False, True):
        for kind, g in gradients(W, H).items():
            routes[(kind, srgb)] = lambda k, g=g, srgb=srgb: fr.layer_paint(ctx, None, 0, 0, frame.data_ptr(), W, H, g, (0, 0, W, H), (0, 0), srgb)
        routes[("rects", srgb)] = lambda k, srgb=srgb: fr.layer_rects(ctx, frame.data_ptr(), W, H, rect, srgb)
    res = {r: [] for r in routes}
    for _ in range(args.repeats + 1):
        for r, fn in routes.items():
            res[r].append(time_calls(ctx, stream, args.calls, fn))
    ms = {r: report("panel", r[0], res[r], W * H, 4, w=W, h=H, srgb=r[1]) for r in routes}
    for srgb in (False, True):
        print(json.dumps({"case": "panel", "w": W, "h": H, "srgb": srgb, "linear_ms_by_rects_ms": round(ms[("linear", srgb)] / ms[("rects", srgb)], 3),
                          "radial_ms_by_linear_ms": round(ms[("radial", srgb)] / ms[("linear", srgb)], 3)}), flush=True)


def text_layers(ctx, args):
    """name -> the layer on the device: bench_layer.py's text-like 3840 x 2160 frame layer and its 4 096 lines"""
    import torch
    font = load_font("DejaVuSans.ttf", allow_hinted=True)
    W, H = 3840, 2160
    gs, places, runs, shape, _, _, lines = workload(font, H // 19, W // 10, 16, seed=5)
    tbuf, plan, dgs, _, _ = render_layer(ctx, gs, places, runs, tuple(shape), lines, 0, 4)
    text = torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda:0")
    h, w = min(H, shape[0]), min(W, shape[1])
    text[:h, :w] = tbuf[:h, :w]
    plan.close()
    dgs.close()
    yield "frame_3840x2160", text
    del text, tbuf
    gs, places, runs, shape, _, _, lines = workload(font, args.lines, 64, 16, seed=16)
    layer, plan, dgs, _, _ = render_layer(ctx, gs, places, runs, (shape[0], (shape[1] + 3) // 4 * 4), lines, 0, 4)
    plan.close()
    dgs.close()
    yield "lines_%d" % args.lines, layer


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50, help="calls per timing")
    ap.add_argument("--repeats", type=int, default=5, help="repeats of each alternated timing")
    ap.add_argument("--lines", type=int, default=4096)
    ap.add_argument("--cases", default="text,panel,big", help="which of text, panel (3840 x 2160) and big (7680 x 4320) to run")
    args = ap.parse_args()
    import torch
    stream = torch.cuda.Stream(device="cuda:0")
    ctx = fr.Context(0, stream.cuda_stream)
    cases = args.cases.split(",")
    if "text" in cases:
        for name, layer in text_layers(ctx, args):
            text_case(ctx, stream, args, name, layer)
    if "panel" in cases:
        panel_case(ctx, stream, args, 3840, 2160)
    if "big" in cases:
        panel_case(ctx, stream, args, 7680, 4320)
    ctx.close()


if __name__ == "__main__":
    main()

"""Warped-composite benchmark: fr_layer_warp, the kernel of csrc/fr_layer_warp.hip, with
tools/bench_layer.py's method: device time per call with its table copy (HIP events on the context's stream around --calls
back-to-back calls), every case and its comparator alternated --repeats times in one process after one warm-up round, the
median with the smallest and largest repeat beside it.  One JSON line per configuration.

  "frame"  bench_layer.py's text-like layer, 3840 x 2160 and 7680 x 4320, over a noise frame of its size, UNORM and sRGB:
           the identity map against fr_layer_over of the same layer ("over_ms"), then the layer turned by 5, 45 and 90
           degrees, zoomed by 2 and shrunk to 0.5 about the frame's middle, the rectangle being the whole frame
  "text"   the README's 4 096 lines of 64 characters at size 16 as a finished layer zoomed by 1.25 per frame, against
           re-rendering the lines at size 20 over the frame with FR_TEXT_LOAD | FR_TEXT_OVER (fr_plan_render_timed)

"bytes_per_px" is the traffic model per pixel of the rectangle: the window pixels the map reaches, each read once (4 bytes
times the window area per rectangle pixel, over the pixels that have a tap), and of the image what the kernel's skip rules
make of the samples per lane group of four, taken from the call's own output over a cleared frame (nothing where the group's
samples are zero, the store alone where every alpha is 255, else load and store).  "tb_per_s" is that over the time,
"ratio" the time over fr_layer_over's and "model_ratio" the two models' bytes over each other.

    python tools/bench_warp.py [--calls 20] [--repeats 5] [--steps 10] [--lines 4096] [--small-only] [--skip-text]"""
import argparse
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]

import font_renderer_amd as fr  # noqa: E402
from bench_layer import bytes_per_px as over_bytes_per_px, render_layer, stats, time_calls  # noqa: E402
from bench_shadow import text_layer  # noqa: E402
from bench_text import workload  # noqa: E402
from fixtures import load_font  # noqa: E402


def about_the_middle(W, H, angle, scale):
    """the forward matrix that turns the W x H layer by `angle` degrees and scales it about its middle, in place"""
    c, s = scale * math.cos(math.radians(angle)), scale * math.sin(math.radians(angle))
    return ((c, -s, W / 2 - c * W / 2 + s * H / 2), (s, c, H / 2 - s * W / 2 - c * H / 2))


def whole_frame(row, W, H):
    """the blit of warp_from_matrix with the whole W x H frame as its rectangle: the same map from the frame's corner"""
    X, Y = row[4], row[5]
    return row[:4] + (0, 0, W, H, row[8] - X * row[10] - Y * row[11], row[9] - X * row[12] - Y * row[13]) + row[10:]


def warp_bytes_per_px(blit, sample):
    """the model: blit a row of make_warp_blits, sample the (rows, cols, 4) u8 output of the blit at o = 255 over a cleared
    frame (the samples themselves)"""
    w, h, W, H = blit[2], blit[3], blit[6], blit[7]
    X, Y = np.arange(0, W, 8, dtype=np.int64)[None, :], np.arange(0, H, 8, dtype=np.int64)[:, None]
    U, V = blit[8] + X * blit[10] + Y * blit[11], blit[9] + X * blit[12] + Y * blit[13]
    hit = ((U >= -32768) & (U < 65536 * w + 32768) & (V >= -32768) & (V < 65536 * h + 32768)).mean()
    area = abs(blit[10] * blit[13] - blit[11] * blit[12]) / 2.0 ** 32           # window pixels per rectangle pixel
    px = sample.reshape(-1, 4, 4)
    live = px.any(axis=(1, 2))
    opaque = (px[..., 3] == 255).all(axis=1)
    return float(4 * area * hit + np.where(live, np.where(opaque, 4, 8), 0).mean())


def frame_case(ctx, stream, args, W, H):
    import torch
    frame = torch.empty((H, W, 4), dtype=torch.uint8, device="cuda:0").random_(0, 256, generator=torch.Generator("cuda:0").manual_seed(W))
    clear = torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda:0")
    text = text_layer(ctx, W, H)
    torch.cuda.synchronize()
    over_blits = fr.make_blits([(0, 0, W, H, 0, 0, 255)])
    maps = {"identity": (0, 1.0), "turn_5": (5, 1.0), "turn_45": (45, 1.0), "turn_90": (90, 1.0), "zoom_2": (0, 2.0), "shrink_0.5": (0, 0.5)}
    rows = {name: whole_frame(fr.warp_from_matrix(about_the_middle(W, H, a, s), (0, 0, W, H)), W, H) for name, (a, s) in maps.items()}
    blits = {name: fr.make_warp_blits([r]) for name, r in rows.items()}
    F, T = frame.data_ptr(), text.data_ptr()
    calls = {}
    for srgb in (False, True):
        calls[("over", srgb)] = lambda k, srgb=srgb: fr.layer_over(ctx, T, W, H, F, W, H, over_blits, srgb)
        for name in maps:
            calls[(name, srgb)] = lambda k, srgb=srgb, name=name: fr.layer_warp(ctx, T, W, H, F, W, H, blits[name], srgb)
    res = {c: [] for c in calls}
    with torch.cuda.stream(stream):
        for _ in range(args.repeats + 1):                               # the first round warms up
            for c, f in calls.items():
                res[c].append(time_calls(ctx, stream, args.calls, f)[0])
    model = {"over": over_bytes_per_px(text.cpu().numpy(), 255)}
    for name in maps:                                                   # the samples: the call itself over a cleared frame
        clear.zero_()
        torch.cuda.synchronize()
        fr.layer_warp(ctx, T, W, H, clear.data_ptr(), W, H, blits[name])
        ctx.sync()
        model[name] = warp_bytes_per_px(rows[name], clear.cpu().numpy())
    for (name, srgb), v in res.items():
        ms, lo, hi = stats(v[1:])
        row = {"case": "frame", "map": name, "path": "over" if name == "over" else "gather", "w": W, "h": H, "srgb": srgb, "ms": round(ms, 4), "min_ms": round(lo, 4),
               "max_ms": round(hi, 4), "bytes_per_px": round(model[name], 2), "tb_per_s": round(W * H * model[name] / (ms * 1e-3) / 1e12, 3), "build": fr.build_id()}
        if name != "over":
            r, rlo, rhi = stats(res[("over", srgb)][1:])
            row.update({"over_ms": round(r, 4), "over_min_ms": round(rlo, 4), "over_max_ms": round(rhi, 4), "ratio": round(ms / r, 3),
                        "model_ratio": round(model[name] / model["over"], 3)})
        print(json.dumps(row), flush=True)


def text_case(ctx, stream, args):
    import torch
    for fi, name in enumerate(["DejaVuSans.ttf", "DejaVuSerif-Italic.ttf"]):
        font = load_font(name, allow_hinted=True)
        gs, places, runs, shape, _, _, lines = workload(font, args.lines, 64, 16, seed=100 * fi + 16)
        zgs, zplaces, zruns, zshape, _, _, zlines = workload(font, args.lines, 64, 20, seed=100 * fi + 16)
        for srgb in (False, True):
            flags = fr.FR_TEXT_SRGB if srgb else 0
            h, w = shape[0], (shape[1] + 3) // 4 * 4
            H, W = max(zshape[0], (5 * h + 3) // 4), (max(zshape[1], (5 * w + 3) // 4) + 3) // 4 * 4
            layer, lplan, dgs, _, _ = render_layer(ctx, gs, places, runs, (h, w), lines, flags, 4)
            lplan.close()
            zcols = np.array([[(225, 105, 180, 255), (40, 200, 90, 255)][s[:k].count(" ") % 2] for s in zlines for k in range(len(s))], np.uint8)
            zdgs = fr.DeviceGlyphSet(ctx, zgs)
            rplan = fr.TextPlanRGBA(zdgs, zplaces, zcols, zruns, None, 4, fr.FR_SAMPLE_CENTER, flags | fr.FR_TEXT_OVER | fr.FR_TEXT_LOAD)
            frame = torch.empty((H, W, 4), dtype=torch.uint8, device="cuda:0").random_(0, 256, generator=torch.Generator("cuda:0").manual_seed(fi))
            torch.cuda.synchronize()

            def warp(k):                                                # the zoom, the layer dragged from frame to frame
                row = fr.warp_from_matrix(((1.25, 0, k % 7 * 0.3), (0, 1.25, k % 5 * 0.7)), (0, 0, w, h))
                fr.layer_warp(ctx, layer.data_ptr(), w, h, frame.data_ptr(), W, H, fr.make_warp_blits([row]), srgb)

            rer, comp = [], []
            with torch.cuda.stream(stream):
                for r in range(args.repeats + 1):
                    a = sorted(rplan.render_timed(frame.data_ptr(), W, H) for _ in range(args.steps))[args.steps // 2]
                    c = time_calls(ctx, stream, args.calls, warp)[0]
                    if r:
                        rer.append(a), comp.append(c)
            (a, alo, ahi), (c, clo, chi) = stats(rer), stats(comp)
            print(json.dumps({"case": "text", "font": name, "lines": args.lines, "srgb": srgb, "layer_mpixel": round(w * h / 1e6, 3), "frame_mpixel": round(W * H / 1e6, 3),
                              "rerender_ms": round(a, 4), "rerender_min_ms": round(alo, 4), "rerender_max_ms": round(ahi, 4), "warp_ms": round(c, 4),
                              "warp_min_ms": round(clo, 4), "warp_max_ms": round(chi, 4), "ratio": round(a / c, 1), "build": fr.build_id()}), flush=True)
            rplan.close()
            zdgs.close()
            dgs.close()
            del layer, frame


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20, help="calls per timing")
    ap.add_argument("--repeats", type=int, default=5, help="repeats of each alternated timing")
    ap.add_argument("--steps", type=int, default=10, help="renders per timing of the text plans")
    ap.add_argument("--lines", type=int, default=4096)
    ap.add_argument("--small-only", action="store_true", help="3840 x 2160 only")
    ap.add_argument("--skip-text", action="store_true", help="case \"frame\" only")
    args = ap.parse_args()
    import torch
    stream = torch.cuda.Stream(device="cuda:0")
    ctx = fr.Context(0, stream.cuda_stream)
    frame_case(ctx, stream, args, 3840, 2160)
    if not args.small_only:
        frame_case(ctx, stream, args, 7680, 4320)
    if not args.skip_text:
        text_case(ctx, stream, args)
    ctx.close()


if __name__ == "__main__":
    main()

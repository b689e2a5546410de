"""Layer-compositing benchmark: fr_layer_over, the bandwidth-bound source-over kernel of
csrc/fr_layer.hip.  Both cases run in one process, the alternatives alternated --repeats times; every figure is the median
over the repeats, with the smallest and largest repeat beside it.  Prints one JSON line per configuration.

Case "frame": a 3840 x 2160 layer over a noise frame (--big adds 7680 x 4320, whose three images no longer fit the
256 MiB Infinity Cache), in the four instances UNORM / sRGB x o = 255 / o = 128, for a fully transparent layer, a
text-like one (lines of text rendered with FR_TEXT_OVER over a transparent clear colour) and a fully opaque one, with
the layer's column on the destination's 16-byte grid and one pixel off it.  "ms" is device time per call: HIP events on
the context's stream around --calls back-to-back calls, so it holds the table upload of each call and any gap the host
leaves; "host_ms" is the host's clock around the same calls up to the stream's end.  "bytes_per_px" is what the kernel's
skip rules make of the layer (4 where the layer is zero, 8 where a' = 255, 12 otherwise), computed here from the
layer's pixels, and "share_of_8TBs" is 12 bytes per pixel over the time against 8 TB/s, the figure the issue asks for:
the kernel's own traffic over the time is "tb_per_s".

Case "text": the README's 4 096 lines of 64 characters (tools/bench_text.py's workload, per-word colours, 16 spp):
re-rendering the lines over the frame with FR_TEXT_LOAD | FR_TEXT_OVER every frame (fr_plan_render_timed) against one
layer render (FR_TEXT_OVER over a transparent clear colour) plus one fr_layer_over per frame, at offsets that change
from frame to frame.  "ratio" is the re-render's time over the composite's, both from this run.

    python tools/bench_layer.py [--calls 50] [--repeats 5] [--steps 10] [--lines 4096] [--big]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]

import font_renderer_amd as fr  # noqa: E402
from bench_text import workload  # noqa: E402
from fixtures import load_font  # noqa: E402

WORDS = [(225, 105, 180, 255), (40, 200, 90, 255)]


def stats(v):
    v = sorted(v)
    return v[len(v) // 2], v[0], v[-1]


def render_layer(ctx, gs, places, runs, shape, lines, flags, samples):
    """the lines as one premultiplied layer of `shape` on the device: FR_TEXT_OVER over clear (0, 0, 0, 0)"""
    import torch
    cols = np.array([WORDS[s[:k].count(" ") % 2] for s in lines for k in range(len(s))], np.uint8)
    dgs = fr.DeviceGlyphSet(ctx, gs)
    plan = fr.TextPlanRGBA(dgs, places, cols, runs, np.zeros((len(runs), 4), np.uint8), samples, fr.FR_SAMPLE_CENTER, flags | fr.FR_TEXT_OVER)
    buf = torch.zeros(shape + (4,), dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    ms = plan.render_timed(buf.data_ptr(), shape[1], shape[0])
    return buf, plan, dgs, cols, ms


def time_calls(ctx, stream, calls, fn):
    """(device ms per call from events on the context's stream, host ms per call up to the stream's end)"""
    import time
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ctx.sync()
    t0 = time.perf_counter()
    e0.record(stream)
    for k in range(calls):
        fn(k)
    e1.record(stream)
    ctx.sync()
    t1 = time.perf_counter()
    return e0.elapsed_time(e1) / calls, (t1 - t0) * 1e3 / calls


def bytes_per_px(layer, o):
    """the kernel's traffic per pixel of `layer` ((rows, cols, 4) u8 on the host) at opacity o, by its skip rules per lane
    group of four pixels: 4 where the group's layer pixels are all zero, 8 where every a' is 255, else 12"""
    px = layer.reshape(-1, 4, 4)
    zero = ~px.any(axis=(1, 2))
    a1 = (px[..., 3].astype(np.int64) * o + 127) // 255
    opaque = (a1 == 255).all(axis=1)
    return float(np.where(zero, 4, np.where(opaque, 8, 12)).mean())


def frame_case(ctx, stream, args, W, H):
    import torch
    gen = torch.Generator("cuda:0").manual_seed(W)
    frame = torch.empty((H, W, 4), dtype=torch.uint8, device="cuda:0").random_(0, 256, generator=gen)
    layers = {"transparent": torch.zeros((H, W + 4, 4), dtype=torch.uint8, device="cuda:0")}
    opaque = torch.empty((H, W + 4, 4), dtype=torch.uint8, device="cuda:0").random_(0, 256, generator=gen)
    opaque[..., 3] = 255
    layers["opaque"] = opaque
    # text-like: lines of text across the frame, rendered by the library itself
    font = load_font("DejaVuSans.ttf", allow_hinted=True)
    gs, places, runs, shape, _, _, lines = workload(font, H // 19, W // 10, 16, seed=5)
    tbuf, plan, dgs, _, _ = render_layer(ctx, gs, places, runs, tuple(shape), lines, 0, 4)
    text = torch.zeros((H, W + 4, 4), dtype=torch.uint8, device="cuda:0")
    h, w = min(H, shape[0]), min(W + 4, shape[1])
    text[:h, :w] = tbuf[:h, :w]
    plan.close()
    dgs.close()
    layers["text"] = text
    torch.cuda.synchronize()
    configs = [(name, srgb, o, off) for name in ("transparent", "text", "opaque") for srgb in (False, True) for o in (255, 128)
               for off in (0, 1)]
    res = {c: [] for c in configs}
    for _ in range(args.repeats + 1):                                   # the first round warms up
        for c in configs:
            name, srgb, o, off = c
            lay = layers[name]
            blits = fr.make_blits([(off, 0, W, H, 0, 0, o)])
            res[c].append(time_calls(ctx, stream, args.calls, lambda k: fr.layer_over(ctx, lay.data_ptr(), W + 4, H, frame.data_ptr(), W, H, blits, srgb)))
    for c in configs:
        name, srgb, o, off = c
        ms, lo, hi = stats([r[0] for r in res[c][1:]])
        host = stats([r[1] for r in res[c][1:]])[0]
        bpp = bytes_per_px(layers[name][:, off:off + W].cpu().numpy(), o)
        print(json.dumps({"case": "frame", "w": W, "h": H, "layer": name, "srgb": srgb, "opacity": o, "src_x": off,
                          "kernel": "fr::layer_over_kernel<%d, %d>" % (srgb, o != 255), "ms": round(ms, 4), "min_ms": round(lo, 4),
                          "max_ms": round(hi, 4), "host_ms": round(host, 4), "bytes_per_px": round(bpp, 2),
                          "tb_per_s": round(W * H * bpp / (ms * 1e-3) / 1e12, 3),
                          "share_of_8TBs": round(W * H * 12 / (ms * 1e-3) / 8e12, 3)}), flush=True)


def text_case(ctx, stream, args):
    import torch
    for fi, name in enumerate(["DejaVuSans.ttf", "DejaVuSerif-Italic.ttf"]):
        font = load_font(name, allow_hinted=True)
        for size in (16, 32):
            gs, places, runs, shape, _, _, lines = workload(font, args.lines, 64, size, seed=100 * fi + size)
            for srgb in (False, True):
                flags = fr.FR_TEXT_SRGB if srgb else 0
                H, W = shape[0], (shape[1] + 3) // 4 * 4                # rows on the 16-byte grid, as a viewer allocates them
                layer, lplan, dgs, cols, _ = render_layer(ctx, gs, places, runs, (H, W), lines, flags, 4)
                rplan = fr.TextPlanRGBA(dgs, places, cols, runs, None, 4, fr.FR_SAMPLE_CENTER, flags | fr.FR_TEXT_OVER | fr.FR_TEXT_LOAD)
                frame = torch.empty((H, W, 4), dtype=torch.uint8, device="cuda:0").random_(0, 256, generator=torch.Generator("cuda:0").manual_seed(size))
                torch.cuda.synchronize()

                def composite(k):
                    fr.layer_over(ctx, layer.data_ptr(), W, H, frame.data_ptr(), W, H, fr.make_blits([(0, 0, W, H, k % 7, k % 5, 255)]), srgb)

                rer, lay, comp, host = [], [], [], []
                for r in range(args.repeats + 1):
                    a = sorted(rplan.render_timed(frame.data_ptr(), W, H) for _ in range(args.steps))[args.steps // 2]
                    b = sorted(lplan.render_timed(layer.data_ptr(), W, H) for _ in range(args.steps))[args.steps // 2]
                    c, hst = time_calls(ctx, stream, args.calls, composite)
                    if r:
                        rer.append(a), lay.append(b), comp.append(c), host.append(hst)
                (a, alo, ahi), (c, clo, chi) = stats(rer), stats(comp)
                print(json.dumps({"case": "text", "font": name, "font_size": size, "lines": args.lines, "srgb": srgb, "mpixel": round(W * H / 1e6, 3),
                                  "rerender_ms": round(a, 4), "rerender_min_ms": round(alo, 4), "rerender_max_ms": round(ahi, 4),
                                  "rerender_plan": rplan.describe(), "layer_render_ms": round(stats(lay)[0], 4),
                                  "composite_ms": round(c, 4), "composite_min_ms": round(clo, 4), "composite_max_ms": round(chi, 4),
                                  "composite_host_ms": round(stats(host)[0], 4),
                                  "composite_bytes_per_px": round(bytes_per_px(layer.cpu().numpy(), 255), 2),
                                  "share_of_8TBs": round(W * H * 12 / (c * 1e-3) / 8e12, 3), "ratio": round(a / c, 1)}), flush=True)
                rplan.close()
                lplan.close()
                dgs.close()
                del layer, frame


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50, help="fr_layer_over calls per timing")
    ap.add_argument("--repeats", type=int, default=5, help="repeats of each alternated timing")
    ap.add_argument("--steps", type=int, default=10, help="renders per timing of the text plans")
    ap.add_argument("--lines", type=int, default=4096)
    ap.add_argument("--big", action="store_true", help="also a 7680 x 4320 frame")
    ap.add_argument("--skip-text", action="store_true", help="case \"frame\" only")
    args = ap.parse_args()
    import torch
    stream = torch.cuda.Stream(device="cuda:0")
    ctx = fr.Context(0, stream.cuda_stream)
    frame_case(ctx, stream, args, 3840, 2160)
    if args.big:
        frame_case(ctx, stream, args, 7680, 4320)
    if not args.skip_text:
        text_case(ctx, stream, args)
    ctx.close()


if __name__ == "__main__":
    main()

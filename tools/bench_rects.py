"""Rectangle benchmark: fr_layer_rects, the tile kernel of csrc/fr_layer_rects.hip, against the
routes a caller had before it.  Everything runs in one process, the alternatives alternated --repeats times; every figure
is the median over the repeats, with the smallest and largest repeat beside it.  "ms" is device time per call: HIP events
on the context's stream around --calls back-to-back calls, so it holds the table upload of each call and any gap the host
leaves.  Prints one JSON line per configuration.

Case "fill": one rectangle over a whole 3840 x 2160 and 7680 x 4320 frame, opaque (the kernel writes 4 bytes per pixel
and reads none) and translucent (8 bytes per pixel: read and write), against fr_layer_over of a solid layer of the same
size (8 and 12 bytes per pixel: it reads the layer too) and, for the opaque one, hipMemsetD32Async of the frame (4).
"tb_per_s" is that traffic model over the time.

Case "lines": the 4 096 lines of tools/bench_text.py, each with a highlight box and an underline: 8 192 rectangles in one
fr_layer_rects call, against the same rectangles rounded to whole pixels as fr_layer_over blits from two solid layers
(two calls: its blits may not overlap, and an underline lies inside its line's box).

    python tools/bench_rects.py [--calls 50] [--repeats 5] [--lines 4096] [--cases fill,big,lines]"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]

import font_renderer_amd as fr  # noqa: E402
from bench_layer import stats, time_calls  # noqa: E402
from bench_text import workload  # noqa: E402
from fixtures import load_font  # noqa: E402


def hip_runtime():
    """the HIP runtime this process already uses (the one PyTorch brought), for hipMemsetD32Async"""
    import torch
    lib = C.CDLL(os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so"))
    lib.hipMemsetD32Async.restype = C.c_int
    lib.hipMemsetD32Async.argtypes = [C.c_void_p, C.c_int, C.c_size_t, C.c_void_p]
    return lib


def report(case, name, res, px, bpp, **extra):
    ms, lo, hi = stats([r[0] for r in res[1:]])                          # the first round warms up
    print(json.dumps({"case": case, "route": name, **extra, "ms": round(ms, 4), "min_ms": round(lo, 4), "max_ms": round(hi, 4),
                      "host_ms": round(stats([r[1] for r in res[1:]])[0], 4), "bytes_per_px": bpp,
                      "tb_per_s": round(px * bpp / (ms * 1e-3) / 1e12, 3)}), flush=True)
    return ms


def fill_case(ctx, stream, hip, args, W, H):
    import torch
    gen = torch.Generator("cuda:0").manual_seed(W)
    frame = torch.empty((H, W, 4), dtype=torch.uint8, device="cuda:0").random_(0, 256, generator=gen)
    frame[..., 3] = 255
    solid = {255: torch.empty((H, W, 4), dtype=torch.uint8, device="cuda:0"), 128: torch.empty((H, W, 4), dtype=torch.uint8, device="cuda:0")}
    solid[255][:] = torch.tensor([200, 60, 250, 255], dtype=torch.uint8, device="cuda:0")
    solid[128][:] = torch.tensor([100, 30, 125, 128], dtype=torch.uint8, device="cuda:0")          # (200, 60, 250) premultiplied by 128
    torch.cuda.synchronize()
    blit = fr.make_blits([(0, 0, W, H, 0, 0, 255)])
    routes = {}
    for srgb in (False, True):
        for A in (255, 128):
            rect = fr.make_rects([(0, 0, 64 * W, 64 * H, (200, 60, 250, A))])
            routes[("rects", srgb, A)] = (lambda k, rect=rect, srgb=srgb: fr.layer_rects(ctx, frame.data_ptr(), W, H, rect, srgb), 4 if A == 255 else 8)
            routes[("over", srgb, A)] = (lambda k, lay=solid[A], srgb=srgb: fr.layer_over(ctx, lay.data_ptr(), W, H, frame.data_ptr(), W, H, blit, srgb),
                                         8 if A == 255 else 12)
    routes[("memset", False, 255)] = (lambda k: hip.hipMemsetD32Async(frame.data_ptr(), 0x7f3cfac8, W * H, stream.cuda_stream), 4)
    res = {r: [] for r in routes}
    for _ in range(args.repeats + 1):
        for r, (fn, _) in routes.items():
            res[r].append(time_calls(ctx, stream, args.calls, fn))
    ms = {r: report("fill", r[0], res[r], W * H, routes[r][1], w=W, h=H, srgb=r[1], alpha=r[2]) for r in routes}
    for srgb in (False, True):
        for A in (255, 128):
            print(json.dumps({"case": "fill", "w": W, "h": H, "srgb": srgb, "alpha": A,
                              "over_ms_by_rects_ms": round(ms[("over", srgb, A)] / ms[("rects", srgb, A)], 3)}), flush=True)


def lines_case(ctx, stream, args):
    import torch
    font = load_font("DejaVuSans.ttf", allow_hinted=True)
    size = 16
    _, places, runs, shape, _, _, _ = workload(font, args.lines, 64, size, seed=size)
    H, W = shape[0], (shape[1] + 3) // 4 * 4
    box, under = font.decoration(size, fr.FR_DECOR_LINE_BOX), font.decoration(size, fr.FR_DECOR_UNDERLINE)
    rects, boxes, lines = [], [], []
    for r in runs:
        base = 64 * (int(r["out_y"]) + int(places[int(r["first"])]["pen_y"]))
        w = int(r["w"])
        rects.append((0, base + box[0], 64 * w, base + box[1], (255, 230, 90, 128)))
        rects.append((0, base + under[0], 64 * w, base + under[1], (40, 60, 220, 255)))
        # the blits: whole pixels, clipped to the line's own rows so that no two of one call overlap
        y0, y1 = max((base + box[0]) // 64, int(r["out_y"])), min(-(-(base + box[1]) // 64), int(r["out_y"]) + int(r["h"]))
        boxes.append((0, 0, w, y1 - y0, 0, y0, 255))
        u0 = (base + under[0]) // 64
        lines.append((0, 0, w, max(1, (under[1] - under[0] + 32) // 64), 0, u0, 255))
    rects, boxes, lines = fr.make_rects(rects), fr.make_blits(boxes), fr.make_blits(lines)
    frame = torch.empty((H, W, 4), dtype=torch.uint8, device="cuda:0").random_(0, 256, generator=torch.Generator("cuda:0").manual_seed(9))
    frame[..., 3] = 255
    lh = int(max(b[3] for b in boxes.tolist()))
    solid_box = torch.empty((lh, W, 4), dtype=torch.uint8, device="cuda:0")
    solid_box[:] = torch.tensor([128, 115, 45, 128], dtype=torch.uint8, device="cuda:0")
    solid_line = torch.empty((lh, W, 4), dtype=torch.uint8, device="cuda:0")
    solid_line[:] = torch.tensor([40, 60, 220, 255], dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    px = sum(int(b[2]) * int(b[3]) for b in boxes.tolist()) + sum(int(b[2]) * int(b[3]) for b in lines.tolist())

    def over(k):
        fr.layer_over(ctx, solid_box.data_ptr(), W, lh, frame.data_ptr(), W, H, boxes)
        fr.layer_over(ctx, solid_line.data_ptr(), W, lh, frame.data_ptr(), W, H, lines)

    routes = {"rects": lambda k: fr.layer_rects(ctx, frame.data_ptr(), W, H, rects), "over": over}
    res = {r: [] for r in routes}
    for _ in range(args.repeats + 1):
        for r, fn in routes.items():
            res[r].append(time_calls(ctx, stream, args.calls, fn))
    ms = {r: report("lines", r, res[r], px, 8 if r == "rects" else 12, lines=args.lines, rectangles=len(rects), mpixel=round(W * H / 1e6, 3)) for r in routes}
    print(json.dumps({"case": "lines", "over_ms_by_rects_ms": round(ms["over"] / ms["rects"], 3)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50, help="calls per timing")
    ap.add_argument("--repeats", type=int, default=5, help="repeats of each alternated timing")
    ap.add_argument("--lines", type=int, default=4096)
    ap.add_argument("--cases", default="fill,big,lines", help="which of fill (3840 x 2160), big (7680 x 4320) and lines to run")
    args = ap.parse_args()
    import torch
    stream = torch.cuda.Stream(device="cuda:0")
    ctx = fr.Context(0, stream.cuda_stream)
    hip = hip_runtime()
    cases = args.cases.split(",")
    if "fill" in cases:
        fill_case(ctx, stream, hip, args, 3840, 2160)
    if "big" in cases:
        fill_case(ctx, stream, hip, args, 7680, 4320)
    if "lines" in cases:
        lines_case(ctx, stream, args)
    ctx.close()


if __name__ == "__main__":
    main()

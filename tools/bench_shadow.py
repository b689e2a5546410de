"""Shadow benchmark: fr_layer_shadow, the stencil kernels of csrc/fr_layer_shadow.hip, on the
text-like layer of tools/bench_layer.py (lines of text rendered with FR_TEXT_OVER over a transparent clear colour) at
3840 x 2160 and 7680 x 4320, UNORM and sRGB, for the parameter sets (s, r, p) = (0, 4, 3), (0, 16, 3), (0, 32, 1), (2, 0, 0).
One process; the cases and their comparators are alternated --repeats times after one warm-up round, and every figure is
the median over the repeats with the smallest and largest repeat beside it.  Prints one JSON line per configuration:

  "ms"            device time per fr_layer_shadow call: HIP events on the context's stream around --calls back-to-back calls
  "over_ms"       (a) fr_layer_over of the same layer over a noise frame of the same size, the streaming comparator: 12 bytes
                  per pixel at most, against this call's 4 read + 4 written + 2 per intermediate stage ("bytes_per_px")
  "avg_pool_ms"   (b) the same number of torch.nn.functional.avg_pool2d passes (stride 1, zero padding) over a float16 alpha
                  plane on the device: a library baseline for time only, its bytes differ (none for the spread-only set)
  "vs_r4_p3", "vs_r4_p1"   (c) the time of radius 32 over the time of radius 4 at three passes and at one (the sets
                  (0, 32, 3) and (0, 4, 1) are timed for this as well), one line per frame size and colour space, which
                  shows how the cost grows with the radius

    python tools/bench_shadow.py [--calls 20] [--repeats 5] [--small-only]"""
import argparse
import json
import os
import sys


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]

import font_renderer_amd as fr  # noqa: E402
from bench_layer import render_layer, stats, time_calls  # noqa: E402
from bench_text import workload  # noqa: E402
from fixtures import load_font  # noqa: E402

SETS = [(0, 4, 3), (0, 16, 3), (0, 32, 1), (2, 0, 0)]
COLOUR = (20, 30, 60, 170)


def text_layer(ctx, W, H):
    """bench_layer.py's text-like layer, W x H on the 16-byte grid"""
    import torch
    font = load_font("DejaVuSans.ttf", allow_hinted=True)
    gs, places, runs, shape, _, _, lines = workload(font, H // 19, W // 10, 16, seed=5)
    tbuf, plan, dgs, _, _ = render_layer(ctx, gs, places, runs, tuple(shape), lines, 0, 4)
    text = torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda:0")
    h, w = min(H, shape[0]), min(W, shape[1])
    text[:h, :w] = tbuf[:h, :w]
    plan.close()
    dgs.close()
    return text


def frame_case(ctx, stream, args, W, H):
    import torch
    import torch.nn.functional as F
    layer = text_layer(ctx, W, H)
    out = torch.empty((H, W, 4), dtype=torch.uint8, device="cuda:0")
    frame = torch.empty((H, W, 4), dtype=torch.uint8, device="cuda:0").random_(0, 256, generator=torch.Generator("cuda:0").manual_seed(W))
    plane = layer[..., 3].to(torch.float16).reshape(1, 1, H, W).contiguous()
    blits = fr.make_blits([(0, 0, W, H, 0, 0, 255)])
    torch.cuda.synchronize()
    sets = SETS + [(0, 32, 3), (0, 4, 1)]
    configs = [(st, srgb) for st in sets for srgb in (False, True)]
    res = {c: [] for c in configs}
    over, pool = {False: [], True: []}, {st: [] for st in sets}

    def shadow(st, srgb):
        s, r, p = st
        return lambda k: fr.layer_shadow(ctx, layer.data_ptr(), W, H, out.data_ptr(), W, H, (0, 0, W, H), (0, 0, W, H), (3, 4), s, r, p, COLOUR, srgb)

    def pooled(st):
        _, r, p = st

        def run(k):
            x = plane
            for _ in range(p):
                x = F.avg_pool2d(x, 2 * r + 1, stride=1, padding=r, count_include_pad=True)
        return run

    with torch.cuda.stream(stream):
        for _ in range(args.repeats + 1):                               # the first round warms up
            for srgb in (False, True):
                over[srgb].append(time_calls(ctx, stream, args.calls, lambda k: fr.layer_over(ctx, layer.data_ptr(), W, H, frame.data_ptr(), W, H, blits, srgb))[0])
            for st in sets:
                if st[1] and st[2]:
                    pool[st].append(time_calls(ctx, stream, args.calls, pooled(st))[0])
                for srgb in (False, True):
                    res[(st, srgb)].append(time_calls(ctx, stream, args.calls, shadow(st, srgb))[0])
    med = {}
    for st, srgb in configs:
        ms, lo, hi = stats(res[(st, srgb)][1:])
        med[(st, srgb)] = ms
        s, r, p = st
        stages = (1 if s else 0) + (p if r else 0)
        row = {"case": "shadow", "w": W, "h": H, "srgb": srgb, "spread": s, "blur_radius": r, "blur_passes": p, "ms": round(ms, 4),
               "min_ms": round(lo, 4), "max_ms": round(hi, 4), "bytes_per_px": 8 + 2 * max(stages - 1, 0),
               "gpx_per_s": round(W * H / (ms * 1e-3) / 1e9, 2), "over_ms": round(stats(over[srgb][1:])[0], 4),
               "vs_over": round(ms / stats(over[srgb][1:])[0], 2)}
        if pool[st]:
            row["avg_pool_ms"] = round(stats(pool[st][1:])[0], 4)
            row["vs_avg_pool"] = round(ms / stats(pool[st][1:])[0], 3)
        print(json.dumps(row), flush=True)
    for srgb in (False, True):
        print(json.dumps({"case": "radius", "w": W, "h": H, "srgb": srgb,
                          "vs_r4_p3": round(med[((0, 32, 3), srgb)] / med[((0, 4, 3), srgb)], 2),
                          "vs_r4_p1": round(med[((0, 32, 1), srgb)] / med[((0, 4, 1), srgb)], 2)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20, help="calls per timing")
    ap.add_argument("--repeats", type=int, default=5, help="repeats of each alternated timing")
    ap.add_argument("--small-only", action="store_true", help="3840 x 2160 only")
    args = ap.parse_args()
    import torch
    stream = torch.cuda.Stream(device="cuda:0")
    ctx = fr.Context(0, stream.cuda_stream)
    frame_case(ctx, stream, args, 3840, 2160)
    if not args.small_only:
        frame_case(ctx, stream, args, 7680, 4320)
    ctx.close()


if __name__ == "__main__":
    main()

"""Outline benchmark: fr_layer_outline, the kernel of csrc/fr_layer_outline.hip, on the text-like
layer of tools/bench_shadow.py at 3840 x 2160 and 7680 x 4320, UNORM and sRGB, FR_OUTLINE_GROW at rho = 16, 24, 64, 128 and
256 (1, 1.5, 4, 8 and 16 pixels).  One process; the cases and their comparator are alternated --repeats times after one
warm-up round, and every figure is the median over the repeats with the smallest and largest repeat beside it.  Prints one
JSON line per configuration:

  "ms"          device time per fr_layer_outline call, its table copy included: HIP events on the context's stream around
                --calls back-to-back calls
  "square_ms"   fr_layer_shadow with spread = ceil(rho / 16) and no blur, for rho <= 128: the square outline of equal
                reach, which is what a caller had before ("vs_square" = ms / square_ms)
  "taps"        the non-zero weights of the disc, the size of the maximum each pixel of a live tile takes

    python tools/bench_outline.py [--calls 20] [--repeats 5] [--small-only] [--kinds]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]

import font_renderer_amd as fr  # noqa: E402
from bench_layer import stats, time_calls  # noqa: E402
from bench_shadow import text_layer  # noqa: E402
from layer_outline_ref import reach, weights  # noqa: E402

RADII = [16, 24, 64, 128, 256]
COLOUR = (20, 30, 60, 230)


def frame_case(ctx, stream, args, W, H):
    import torch
    layer = text_layer(ctx, W, H)
    out = torch.empty((H, W, 4), dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    kinds = (0, 1, 2, 3) if args.kinds else (0,)
    configs = [(rho, kind, srgb) for rho in RADII for kind in kinds for srgb in (False, True)]
    res = {c: [] for c in configs}
    square = {(rho, srgb): [] for rho in RADII if rho <= 128 for srgb in (False, True)}

    def outline(rho, kind, srgb):
        return lambda k: fr.layer_outline(ctx, layer.data_ptr(), W, H, out.data_ptr(), W, H, (0, 0, W, H), (0, 0, W, H), (0, 0), rho, kind, COLOUR, srgb)

    def spread(rho, srgb):
        return lambda k: fr.layer_shadow(ctx, layer.data_ptr(), W, H, out.data_ptr(), W, H, (0, 0, W, H), (0, 0, W, H), (0, 0), reach(rho), 0, 0, COLOUR, srgb)

    with torch.cuda.stream(stream):
        for _ in range(args.repeats + 1):                               # the first round warms up
            for rho, kind, srgb in configs:
                res[(rho, kind, srgb)].append(time_calls(ctx, stream, args.calls, outline(rho, kind, srgb))[0])
                if kind == 0 and rho <= 128:
                    square[(rho, srgb)].append(time_calls(ctx, stream, args.calls, spread(rho, srgb))[0])
    for rho, kind, srgb in configs:
        ms, lo, hi = stats(res[(rho, kind, srgb)][1:])
        row = {"case": "outline", "w": W, "h": H, "srgb": srgb, "radius": rho, "kind": kind, "taps": int((weights(rho) > 0).sum()), "ms": round(ms, 4),
               "min_ms": round(lo, 4), "max_ms": round(hi, 4), "gpx_per_s": round(W * H / (ms * 1e-3) / 1e9, 2)}
        if kind == 0 and rho <= 128:
            sq, sq_lo, sq_hi = stats(square[(rho, srgb)][1:])
            row.update({"square_ms": round(sq, 4), "square_min_ms": round(sq_lo, 4), "square_max_ms": round(sq_hi, 4), "vs_square": round(ms / sq, 2)})
        print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20, help="calls per timing")
    ap.add_argument("--repeats", type=int, default=5, help="repeats of each alternated timing")
    ap.add_argument("--small-only", action="store_true", help="3840 x 2160 only")
    ap.add_argument("--kinds", action="store_true", help="all four kinds, not FR_OUTLINE_GROW alone")
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

"""Blend-mode benchmark: fr_layer_blend, the kernels of csrc/fr_layer_blend.hip, with
tools/bench_layer.py's method: device time per call with its table copy (HIP events on the context's stream around --calls
back-to-back calls), every mode and fr_layer_over of the same layer alternated --repeats times in one process after one
warm-up round, the median with the smallest and largest repeat beside it.  The text-like layer of bench_layer.py over a
noise frame, 3840 x 2160 and 7680 x 4320, UNORM and sRGB.  One JSON line per configuration.

"bytes_per_px" is the traffic model, computed here from the pixels per lane group of four: a blend moves 4 bytes per pixel
where the group's layer pixels are all zero and 12 elsewhere (it needs the destination under an opaque pixel too);
fr_layer_over moves 4, 8 where every a' is 255, else 12.  "tb_per_s" is that over the time, "ratio" the time over
fr_layer_over's and "model_ratio" the two models' bytes over each other.  The frame is blended into again and again, so its
bytes drift (MULTIPLY darkens it); no kernel's work depends on the destination's values.

    python tools/bench_blend.py [--calls 20] [--repeats 5] [--small-only] [--modes multiply,overlay,plus]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]

import font_renderer_amd as fr  # noqa: E402
from bench_layer import bytes_per_px as over_bytes_per_px, stats, time_calls  # noqa: E402
from bench_shadow import text_layer  # noqa: E402

NAMES = ("multiply", "screen", "overlay", "darken", "lighten", "hard_light", "difference", "exclusion", "plus")


def blend_bytes_per_px(layer):
    """4 where a lane group's four layer pixels are all zero, else 12.  layer (rows, cols, 4) u8 on the host."""
    zero = ~layer.reshape(-1, 4, 4).any(axis=(1, 2))
    return float(np.where(zero, 4, 12).mean())


def frame_case(ctx, stream, args, W, H):
    import torch
    frame = torch.empty((H, W, 4), dtype=torch.uint8, device="cuda:0").random_(0, 256, generator=torch.Generator("cuda:0").manual_seed(W))
    text = text_layer(ctx, W, H)
    torch.cuda.synchronize()
    blits = fr.make_blits([(0, 0, W, H, 0, 0, 255)])
    F, T = frame.data_ptr(), text.data_ptr()
    modes = [NAMES.index(m) for m in args.modes.split(",")]
    calls = {}
    for srgb in (False, True):
        calls[("over", srgb)] = lambda k, srgb=srgb: fr.layer_over(ctx, T, W, H, F, W, H, blits, srgb)
        for mode in modes:
            calls[(NAMES[mode], srgb)] = lambda k, srgb=srgb, mode=mode: fr.layer_blend(ctx, T, W, H, F, W, H, blits, mode, srgb)
    res = {c: [] for c in calls}
    with torch.cuda.stream(stream):
        for _ in range(args.repeats + 1):                               # the first round warms up
            for c, f in calls.items():
                res[c].append(time_calls(ctx, stream, args.calls, f)[0])
    text_h = text.cpu().numpy()
    model = {"over": over_bytes_per_px(text_h, 255), "blend": blend_bytes_per_px(text_h)}
    for (name, srgb), v in res.items():
        ms, lo, hi = stats(v[1:])
        bpp = model["over" if name == "over" else "blend"]
        row = {"case": name, "w": W, "h": H, "srgb": srgb, "ms": round(ms, 4), "min_ms": round(lo, 4), "max_ms": round(hi, 4),
               "bytes_per_px": round(bpp, 2), "tb_per_s": round(W * H * bpp / (ms * 1e-3) / 1e12, 3), "build": fr.build_id()}
        if name != "over":
            r, rlo, rhi = stats(res[("over", srgb)][1:])
            row.update({"over_ms": round(r, 4), "over_min_ms": round(rlo, 4), "over_max_ms": round(rhi, 4), "ratio": round(ms / r, 3),
                        "model_ratio": round(bpp / model["over"], 3)})
        print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20, help="calls per timing")
    ap.add_argument("--repeats", type=int, default=5, help="repeats of each alternated timing")
    ap.add_argument("--small-only", action="store_true", help="3840 x 2160 only")
    ap.add_argument("--modes", default="multiply,overlay,plus")
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

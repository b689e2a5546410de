"""Masked-composite benchmark: fr_layer_mask, the kernel of csrc/fr_layer_mask.hip, with
tools/bench_layer.py's method: device time per call with its table copy (HIP events on the context's stream around --calls
back-to-back calls), every case and its comparator alternated --repeats times in one process after one warm-up round, the
median with the smallest and largest repeat beside it.  3840 x 2160 and 7680 x 4320, UNORM and sRGB.  One JSON line per
configuration.

  "frame"  the text-like layer of bench_layer.py through a full-frame rounded panel (255 inside, soft corners and edges, a
           margin of 0), as a layer mask and as a plane, against fr_layer_over of the same layer ("over_ms")
  "clip"   the same with the right half of the mask 0: the workload on which a kernel whose layer loads wait for the mask
           was weighed against the one kept
  "solid"  an opaque one-colour layer through the text layer's alpha against fr_layer_paint with one stop through the same
           layer ("paint_ms"): the same bytes by consequence 4
  "erase"  FR_MASK_ERASE of the frame through the text layer against fr_layer_over of that layer

"bytes_per_px" is the traffic model: what the kernel's skip rules make of the images, per lane group of four pixels, the
mask's 4 bytes (layer) or 1 byte (plane) per pixel included, computed here from the pixels; "tb_per_s" is that over the time,
"ratio" the time over the comparator's and "model_ratio" the two models' bytes over each other.

    python tools/bench_mask.py [--calls 20] [--repeats 5] [--small-only] [--cases frame,clip,solid,erase]"""
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


def m(x, y):
    return (x.astype(np.int64) * y + 127) // 255


def mask_bytes_per_px(layer, k, o, mask_bytes):
    """the composite's traffic per pixel by its skip rules per group of four: the mask, the layer, nothing of the image where
    no pixel has t != 0 and a layer pixel != 0, its store alone where every a' is 255, else load and store.  layer (rows,
    cols, 4) u8, k (rows, cols) u8 on the host."""
    t = m(k, o).reshape(-1, 4)
    px = layer.reshape(-1, 4, 4)
    live = ((px.any(axis=2)) & (t != 0)).any(axis=1)
    opaque = (m(px[..., 3], t) == 255).all(axis=1)
    return float((mask_bytes + 4 + np.where(live, np.where(opaque, 4, 8), 0)).mean())


def erase_bytes_per_px(k, o, mask_bytes):
    t = m(k, o).reshape(-1, 4)
    return float((mask_bytes + np.where((t != 0).any(axis=1), np.where((t == 255).all(axis=1), 4, 8), 0)).mean())


def panel(W, H, half=False):
    """the rounded panel's alpha (rows, cols) u8 on the device: 255 inside, 0 in a margin of 64 pixels, corners of radius 96
    and edges 8 pixels soft; half: 0 over the right half of the frame too"""
    import torch
    margin, radius, soft = 64.0, 96.0, 8.0
    x = torch.arange(W, device="cuda:0", dtype=torch.float32)[None, :] + 0.5
    y = torch.arange(H, device="cuda:0", dtype=torch.float32)[:, None] + 0.5
    dx = torch.clamp(torch.maximum(margin + radius - x, x - (W - margin - radius)), min=0.0)
    dy = torch.clamp(torch.maximum(margin + radius - y, y - (H - margin - radius)), min=0.0)
    a = torch.clamp((radius - torch.sqrt(dx * dx + dy * dy)) / soft + 0.5, 0.0, 1.0)
    if half:
        a[:, W // 2:] = 0.0
    return torch.round(a * 255.0).to(torch.uint8).contiguous()


def frame_case(ctx, stream, args, W, H):
    import torch
    gen = torch.Generator("cuda:0").manual_seed(W)
    frame = torch.empty((H, W, 4), dtype=torch.uint8, device="cuda:0").random_(0, 256, generator=gen)
    text = text_layer(ctx, W, H)
    solid = torch.empty((H, W, 4), dtype=torch.uint8, device="cuda:0")
    solid[:] = torch.tensor([200, 10, 99, 255], dtype=torch.uint8, device="cuda:0")
    planes = {"frame": panel(W, H), "clip": panel(W, H, True)}
    layers = {}
    for name, p in planes.items():
        lay = torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda:0")
        lay[..., 3] = p
        layers[name] = lay
    torch.cuda.synchronize()
    whole = fr.make_mask_blits([(0, 0, W, H, 0, 0, 0, 0, 255, 0)])
    over_blits = fr.make_blits([(0, 0, W, H, 0, 0, 255)])
    grad = fr.make_gradient_linear(0, 0, 64, 0, [(0, (200, 10, 99, 255))])
    F, T = frame.data_ptr(), text.data_ptr()

    def mask_call(src, msk, stride, srgb, plane=False, erase=False):
        return lambda k: fr.layer_mask(ctx, src, W, H, msk, stride, H, F, W, H, whole, srgb, plane, erase)

    calls = {}
    for srgb in (False, True):
        calls[("over", "", srgb)] = lambda k, srgb=srgb: fr.layer_over(ctx, T, W, H, F, W, H, over_blits, srgb)
        for case in ("frame", "clip"):
            calls[(case, "layer", srgb)] = mask_call(T, layers[case].data_ptr(), W, srgb)
            calls[(case, "plane", srgb)] = mask_call(T, planes[case].data_ptr(), W, srgb, plane=True)
        calls[("solid", "layer", srgb)] = mask_call(solid.data_ptr(), T, W, srgb)
        calls[("paint", "", srgb)] = lambda k, srgb=srgb: fr.layer_paint(ctx, T, W, H, F, W, H, grad, (0, 0, W, H), (0, 0), srgb)
        calls[("erase", "layer", srgb)] = mask_call(None, T, W, srgb, erase=True)
    wanted = set(args.cases.split(","))
    calls = {c: f for c, f in calls.items() if c[0] in wanted or (c[0] == "over" and wanted & {"frame", "clip", "erase"}) or (c[0] == "paint" and "solid" in wanted)}
    res = {c: [] for c in calls}
    with torch.cuda.stream(stream):
        for _ in range(args.repeats + 1):                               # the first round warms up
            for c, f in calls.items():
                res[c].append(time_calls(ctx, stream, args.calls, f)[0])
    # the traffic models, from the pixels
    text_h = text.cpu().numpy()
    alpha = np.ascontiguousarray(text_h[..., 3])
    solid_h = solid.cpu().numpy()
    model = {("over", ""): over_bytes_per_px(text_h, 255)}
    model[("paint", "")] = mask_bytes_per_px(solid_h, alpha, 255, 4) - 4       # the gradient reads no layer beside the mask
    for case in ("frame", "clip"):
        k = planes[case].cpu().numpy()
        for kind, nbytes in (("layer", 4), ("plane", 1)):
            model[(case, kind)] = mask_bytes_per_px(text_h, k, 255, nbytes)
    model[("solid", "layer")] = mask_bytes_per_px(solid_h, alpha, 255, 4)
    model[("erase", "layer")] = erase_bytes_per_px(alpha, 255, 4)
    for (case, kind, srgb), v in res.items():
        ms, lo, hi = stats(v[1:])
        bpp = model[(case, kind)]
        row = {"case": case, "mask": kind, "w": W, "h": H, "srgb": srgb, "ms": round(ms, 4), "min_ms": round(lo, 4), "max_ms": round(hi, 4),
               "bytes_per_px": round(bpp, 2), "tb_per_s": round(W * H * bpp / (ms * 1e-3) / 1e12, 3), "build": fr.build_id()}
        ref = {"frame": "over", "clip": "over", "erase": "over", "solid": "paint"}.get(case)
        if ref:
            r, rlo, rhi = stats(res[(ref, "", srgb)][1:])
            row.update({ref + "_ms": round(r, 4), ref + "_min_ms": round(rlo, 4), ref + "_max_ms": round(rhi, 4), "ratio": round(ms / r, 3),
                        "model_ratio": round(bpp / model[(ref, "")], 3)})
        print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20, help="calls per timing")
    ap.add_argument("--repeats", type=int, default=5, help="repeats of each alternated timing")
    ap.add_argument("--small-only", action="store_true", help="3840 x 2160 only")
    ap.add_argument("--cases", default="frame,clip,solid,erase")
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

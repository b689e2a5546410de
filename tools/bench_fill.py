#!/usr/bin/env python3
"""Cost of FR_FILL_CONSISTENT: the same plan rendered with flags = 0 and with the flag, interleaved, on the C3 shape
(20 992 synthetic glyphs of 128 segments, 256^2 cells, 16 samples per pixel) and on DejaVuSerif-Italic's whole font
(256^2 cells, 16 samples, and the gray map).  Kernel time per render (events around fr_plan_render), median of N."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np, torch
import font_renderer_amd as fr
from font_renderer_amd.atlas import atlas_shape, cell_jobs
from font_renderer_amd.synth import synth_glyphset
from fixtures import load_font

N = int(sys.argv[1]) if len(sys.argv) > 1 else 20
stream = torch.cuda.Stream()
ctx = fr.Context(0, stream.cuda_stream)
font = load_font("DejaVuSerif-Italic.ttf")
cases = [("c3_cjk21k_256px_s128_16spp", synth_glyphset(20992, 128), 2048, 256, fr.FR_COVERAGE_U8, 4),
         ("dejavuserif_italic_256px_16spp", font.glyphset()[0], font.information.units_per_em, 230, fr.FR_COVERAGE_U8, 4),
         ("dejavuserif_italic_256px_gray_debug", font.glyphset()[0], font.information.units_per_em, 230, fr.FR_GRAY_DEBUG, 1)]
for name, gs, upm, size, mode, n in cases:
    dgs = fr.DeviceGlyphSet(ctx, gs)
    H, W = atlas_shape(len(gs), 256, 64)
    jobs = cell_jobs(gs, 256, size, upm, 64)
    with torch.cuda.stream(stream):
        out = torch.zeros((H, W), dtype=torch.uint8, device="cuda")
    plans = {f: fr.Plan(dgs, jobs, mode, n, fr.FR_SAMPLE_CENTER if n > 1 else fr.FR_SAMPLE_CORNER, f) for f in (0, fr.FR_FILL_CONSISTENT)}
    t = {f: [] for f in plans}
    for _ in range(3):
        for p in plans.values():
            p.render_timed(out.data_ptr(), W, H)
    for _ in range(N):
        for f, p in plans.items():
            t[f].append(p.render_timed(out.data_ptr(), W, H))
    m0, m1 = np.median(t[0]), np.median(t[fr.FR_FILL_CONSISTENT])
    print(f"{name:40s} flags=0 {m0:8.4f} ms   FR_FILL_CONSISTENT {m1:8.4f} ms   {100 * (m1 / m0 - 1):+6.2f} %   "
          f"({plans[fr.FR_FILL_CONSISTENT].describe()})", flush=True)
    for p in plans.values():
        p.close()
    dgs.close()

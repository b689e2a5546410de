#!/usr/bin/env python3
"""Host cost of one fr_plan_render call on a text plan, for ONE library build (FR_RASTER_LIB picks it; default: the
product): the plan of tests/text_instance_cases.py (one run, three placements, coverage, 4 x 4 samples) and its
FR_TEXT_CACHE twin.  Per plan: 300 batches of 20 calls, the stream drained outside the timed span; prints the median
batch's time per call.  Compare two builds with fresh processes run alternately in one session."""
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import fixtures  # noqa: E402
import font_renderer_amd as fr  # noqa: E402
import text_instance_cases as T  # noqa: E402
from font_renderer_amd import _lib as L  # noqa: E402

lib = L.load_library()
import importlib.util  # noqa: E402
# (the runtime load_library bound to: the output is a plain hipMalloc, so no torch import is in the process)
hip = C.CDLL(os.path.join(list(importlib.util.find_spec("torch").submodule_search_locations)[0], "lib", "libamdhip64.so"))
with fr.Context(0) as ctx:
    buf = C.c_void_p()
    assert hip.hipMalloc(C.byref(buf), C.c_size_t(T.SHAPE[0] * T.SHAPE[1])) == 0
    dgs = fr.DeviceGlyphSet(ctx, T.glyph_set(fixtures.load_ascii()))
    out = []
    for flags in (0, fr.FR_TEXT_CACHE):
        plan = fr.TextPlan(dgs, T.places_of(0), T.runs(), fr.FR_COVERAGE_U8, 4, fr.FR_SAMPLE_CORNER, flags)
        render = lambda: plan.render(buf.value, T.SHAPE[1], T.SHAPE[0])
        for _ in range(2000):
            render()
        ctx.sync()
        per_call = []
        for _ in range(300):
            t = time.perf_counter()
            for _ in range(20):
                render()
            per_call.append((time.perf_counter() - t) / 20 * 1e6)
            ctx.sync()
        out.append(f"{'cached' if flags else 'plain'} {statistics.median(per_call):.2f} us ({plan.describe()})")
        plan.close()
    dgs.close()
    assert hip.hipFree(buf) == 0
print(f"{os.path.basename(os.path.dirname(L.lib_path()))}/{os.path.basename(L.lib_path())}: " + "; ".join(out))

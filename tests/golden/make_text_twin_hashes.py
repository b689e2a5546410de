#!/usr/bin/env python3
"""Mint tests/golden/text_twin_hashes.json from the CPU twins of the text path: SHA-256 and shape of what they compute
over one small case, the colour case of tests/test_gpu_text_over.py.  The file pins the twins themselves, so that a change
to them shows as a change of their output and not only through the kernels they judge.  compute(group) is what
tests/test_text_twin_golden.py recomputes, group by group."""
import functools
import hashlib
import json
import math
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))]

import text_twin as tw  # noqa: E402

GRIDS = [(4, True, False), (2, False, True), (1, True, False)]              # (n, centre phase, fill)
SENT = 0x5b
GROUPS = ([("gray", form) for form in tw.FORMS] + [("geometry", form) for form in tw.FORMS] + [("srgb_tables",)]
          + [("rgba", form, n, srgb, load) for form in tw.FORMS for n, _, _ in GRIDS for srgb in (False, True) for load in (False, True)])


def _cell(form, gs, pl, run, widen=0):
    if form == "plain":
        g, px, py, s = tw.plain_place_params(pl, run)
        return tw.plain_cell(gs.boxes[g], s, px, py)
    if form == "ex":
        g, px, py, s, k = tw.ex_place_params(pl, run)
        return tw.ex_cell(gs.boxes[g], s, k, px, py, widen)
    g, px, py, m = tw.affine_place_params(pl)
    return tw.affine_cell(gs.boxes[g], m, px, py, widen)


@functools.lru_cache(maxsize=None)
def colour_case():
    """the colour case of tests/test_gpu_text_over.py: six overlapping italic glyphs at size 21 in two runs of 200 x 27 with
    the placements in both orders, in the three placement forms; translucent colours with one A = 255 and one A = 0; clear
    colours with alpha 128 and 255; noise with random alpha for LOAD"""
    from fixtures import load_font
    from font_renderer_amd import render_glyph as rg
    font = load_font("DejaVuSerif-Italic.ttf")
    gi, pen, _ = font.layout("fjfjWf", 21)
    gs, kept = font.glyphset(sorted({int(g) for g in gi}), skip_unsupported=False)
    local = {g: k for k, g in enumerate(kept)}
    scale = np.float32(21) / np.float32(font.information.units_per_em)
    xs = 64 * 4 + 16 + 192 * np.arange(6)
    fwd = [(local[int(g)], int(x), 20) for g, x in zip(gi, xs)]
    rows = fwd + fwd[::-1]
    plain = rg.make_places(rows)
    ex = rg.make_places_ex([(g, x, 64 * y + 24, 0.0, 0.2) for g, x, y in rows])
    c, s = math.cos(math.radians(33.0)), math.sin(math.radians(33.0))
    m = tuple(float(np.float32(v)) for v in (float(scale) * c, -float(scale) * s, float(scale) * s, float(scale) * c))
    affine = rg.make_places_affine([(g, x, 64 * y) + m for g, x, y in rows])
    runs = rg.make_runs([(0, 6, 200, 27, 1, 1, scale), (6, 6, 200, 27, 1, 29, scale)])
    shape = (57, 202)
    rng = np.random.default_rng(5)
    translucent = rng.integers(0, 256, (12, 4)).astype(np.uint8)
    translucent[0, 3], translucent[7, 3] = 255, 0
    clears = np.array([(10, 60, 90, 128), (255, 255, 240, 255)], np.uint8)
    noise = rng.integers(0, 256, shape + (4,)).astype(np.uint8)
    return dict(gs=gs, places={"plain": plain, "ex": ex, "affine": affine}, runs=runs, shape=shape, translucent=translucent,
                clears=clears, noise=noise, sent=np.full(shape + (4,), SENT, np.uint8))


def _h(a):
    a = np.ascontiguousarray(a)
    return {"sha256": hashlib.sha256(a.tobytes()).hexdigest(), "shape": list(a.shape)}


def _gray(case, form):
    gs, places, runs = case["gs"], case["places"][form], case["runs"]
    out = {}
    for n, center, fill in GRIDS:
        img = tw.render_runs(form, gs, places, runs, np.full(case["shape"], SENT, np.uint8), n, center, fill)
        out[f"gray/{form}/n{n}"] = _h(img)
    if form == "plain":
        img = tw.render_runs(form, gs, places, runs, np.full(case["shape"], SENT, np.uint8), 4, True, False, which=[1])
        out["gray/plain/n4/which1"] = _h(img)
    out[f"gray/{form}/mask"] = _h(tw.to_bytes(tw.coverage_samples(form, gs, places, runs[0], 1, True, False), 1))
    return out


def _geometry(case, form):
    gs, places, runs = case["gs"], case["places"][form], case["runs"]
    out = {}
    for widen in ((0,) if form == "plain" else (0, 1)):
        cells = [[int(v) for v in _cell(form, gs, places[idx], run, widen)]
                 for run in runs for idx in range(int(run["first"]), int(run["first"]) + int(run["count"]))]
        out[f"geometry/{form}/cell/widen{widen}"] = cells
    out[f"geometry/{form}/met_tiles"] = sorted(list(t) for t in tw.met_tiles(form, gs, places, runs))
    if form == "affine":
        out["geometry/affine/inverse"] = [[float(v).hex() for v in tw.inverse(pl["m"])] for pl in places]
    if form == "ex":
        out["geometry/ex/from_ex"] = _h(np.asarray(tw.from_ex(places, runs)).view(np.uint8))
    return out


def _rgba(case, form, n, srgb, load):
    gs, places, runs, cols = case["gs"], case["places"][form], case["runs"], case["translucent"]
    (_, center, fill), = [g for g in GRIDS if g[0] == n]
    clears, start = (None, case["noise"]) if load else (case["clears"], case["sent"])
    out = {}
    for bgr in (False, True):
        key = f"rgba/{form}/n{n}/{'srgb' if srgb else 'unorm'}/{'load' if load else 'clear'}/{'bgra' if bgr else 'rgba'}"
        out[key] = _h(tw.rgba_render_runs(form, gs, places, cols, runs, clears, start.copy(), n, center, fill, srgb, bgr, load))
        out[key + "/over"] = _h(tw.over_render_runs(form, gs, places, cols, runs, clears, start, n, center, fill, srgb, bgr, load))
    return out


def compute(group):
    """the entries of one group of GROUPS -> {key: value}"""
    kind, args = group[0], group[1:]
    if kind == "srgb_tables":
        return {"srgb_tables/D": _h(tw.D.astype("<i8")), "srgb_tables/E": _h(tw.E.astype("<i8"))}
    return {"gray": _gray, "geometry": _geometry, "rgba": _rgba}[kind](colour_case(), *args)


if __name__ == "__main__":
    pins = {}
    for group in GROUPS:
        pins.update(compute(group))
    with open(os.path.join(HERE, "text_twin_hashes.json"), "w") as f:
        f.write("{\n" + ",\n".join(" %s: %s" % (json.dumps(k), json.dumps(pins[k], sort_keys=True)) for k in sorted(pins)) + "\n}\n")
    print(len(pins), "entries")

#!/usr/bin/env python3
"""Mint tests/golden/text_line_pins.json from the line builders of font_renderer_amd.text: what _line, span_line,
view_line, rotated_line and decoration_rects return for a few strings in two fonts at three sizes, as the SHA-256 of the
placement and run tables, the placements' dtype, the image size and the colours.  The builders are host arithmetic over
the library's layout, so the file pins them without a device, and a rewrite of them shows as a change of what they
return.  compute(group) is what tests/test_text_line_pins.py recomputes, group by group."""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))]

FONTS = ("DejaVuSans.ttf", "DejaVuSerif-Italic.ttf")
SIZES = (11, 19, 40)
STRINGS = {"pangram": "The quick brown fox", "overlap": "fjfjWf", "spaces": "   ", "left": "jJoy"}  # j reaches left of the pen
SLANTS = (0.0, 0.2, -0.35)
VIEWS = ((1.37, 3.3, 20.7, 0.0), (0.6, -2.125, 9.5, 0.2))                   # (zoom, offset_x, offset_y, slant)
ANGLES = (0.0, 33.0, 90.0, 217.5)
COLOURS = ((200, 30, 40), (10, 220, 30, 128), (1, 2, 3, 0))
GROUPS = [(name, size) for name in FONTS for size in SIZES]


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _tables(line):
    """(glyph set, places, runs, ...) or None -> what is pinned of it"""
    if line is None:
        return None
    gs, places, runs = line[:3]
    out = {"glyphs": _sha(gs.points_xy) + _sha(gs.contour_start) + _sha(gs.glyph_start) + _sha(gs.boxes),
           "places": _sha(places), "runs": _sha(runs), "descr": places.dtype.descr}
    if len(line) > 3:
        out["width"], out["height"] = int(line[3]), int(line[4])
    if len(line) > 5:
        out["colours"] = [list(c) for c in line[5]]
    return out


def compute(group):
    """the entries of one (font, size) -> {key: value}"""
    from fixtures import load_font
    from font_renderer_amd import text as T
    name, size = group
    font = load_font(name, allow_hinted=True)
    small = (3 * size + 3) // 5
    out = {}
    for label, s in STRINGS.items():
        key = f"{name}/{size}/{label}"
        for k in SLANTS:
            out[f"{key}/line/{k}"] = _tables(T._line(font, s, size, k))
        a, b = len(s) // 3, 2 * len(s) // 3
        spans = [(s[:a], size, 0.0, 0.0, COLOURS[0]), (s[a:b], size, 0.2, -1.5, COLOURS[1]), (s[b:], small, -0.35, 2.26, COLOURS[2])]
        out[f"{key}/spans"] = _tables(T.span_line(font, spans))
        for zoom, ox, oy, k in VIEWS:
            out[f"{key}/view/{zoom}/{k}"] = _tables(T.view_line(font, s, size, zoom, ox, oy, 300, 70, k))
        for angle in ANGLES:
            for k in (0.0, 0.2):
                out[f"{key}/rotated/{angle}/{k}"] = _tables(T.rotated_line(font, s, size, angle, 150.3, 99.77, 300, 200, 1.25, k))
        rows = T.decoration_rects(font, s, size, 3.3, 20.7, underline=COLOURS[0], strikeout=COLOURS[1], highlight=COLOURS[2])
        out[f"{key}/decoration"] = [[float(v).hex() for v in r[:4]] + [list(r[4])] for r in rows]
    return json.loads(json.dumps(out))


if __name__ == "__main__":
    pins = {}
    for group in GROUPS:
        pins.update(compute(group))
    with open(os.path.join(HERE, "text_line_pins.json"), "w") as f:
        f.write("{\n" + ",\n".join(" %s: %s" % (json.dumps(k), json.dumps(pins[k], sort_keys=True)) for k in sorted(pins)) + "\n}\n")
    print(len(pins), "entries")

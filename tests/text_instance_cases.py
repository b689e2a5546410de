"""One tiny text plan per text kernel instance a plan can launch (tests/test_gpu_text_instances.py): 234 keys (form,
colour family, N, FILL, BLEND) of the three placement forms, and 39 FR_TEXT_CACHE keys (colour family, N, BLEND), each
with the fill rule and the form of one of its plain twins, chosen so that the 39 between them reach all six
glyph_mask_kernel<N, FILL> instances.

Every case is the same picture: two fixture glyphs, three overlapping placements, one run of 70 x 20 pixels at (3, 2) of a
25 x 77 buffer, so the run spans two 64 x 16 tiles each way, the last placement's cell crosses both tile edges and is
clipped at the run's right edge, and a border of the start value surrounds the run.  Corner phase: the sample row (or,
under the quarter turn of the affine form, the sample column) through the pen of placement 0 lies exactly on the baseline
vertices of STIX 'A', where FR_FILL_CONSISTENT changes pixels (tests/test_gpu_fill_rule.py: test_render_glyph_ex), for
every N.  The _ex placements are slanted and two of them have a baseline fraction; the affine ones are turned."""
import math
from collections import namedtuple

import numpy as np

import font_renderer_amd as fr
from font_renderer_amd import render_glyph as rg
from font_renderer_amd.glyph import GlyphSet

FORMS = ("", "place_", "affine_")                      # as the kernels' names spell them
FAMILIES = ("", "rgba_", "srgb_", "rgba_load_", "srgb_load_")
SENT = 0x5b
SHAPE = (25, 77)
RUN = (0, 3, 70, 20, 3, 2)                             # first, count, w, h, out_x, out_y
SCALE = np.float32(0.024)
OPAQUE = [(225, 105, 180, 255), (30, 200, 90, 255), (250, 240, 20, 255)]
TRANSLUCENT = [(225, 105, 180, 128), (30, 200, 90, 200), (250, 240, 20, 77)]
CLEAR = [(10, 20, 30, 40)]

Key = namedtuple("Key", "cached form fam n fill blend")


def key_id(k):
    return f"{'cached' if k.cached else 'plain'}/{FORMS[k.form]}{FAMILIES[k.fam]}n{k.n}/fill{k.fill}/blend{k.blend}"


def plain_keys():
    out = []
    for form in range(3):
        for fam in range(5):
            for n in (1, 2, 4):
                for fill in (0, 1):
                    for blend in ((0,) if fam == 0 else (0, 1, 2)):
                        out.append(Key(False, form, fam, n, fill, blend))
    return out


def cached_keys():
    """each with the fill rule and the form (plain or _ex: the affine form has no cache) of one plain twin, alternating"""
    out = []
    for fam in range(5):
        for n in (1, 2, 4):
            for blend in ((0,) if fam == 0 else (0, 1, 2)):
                out.append(Key(True, len(out) // 2 % 2, fam, n, len(out) % 2, blend))
    return out


def twin_of(k):
    return k._replace(cached=False)


def glyph_set(ascii_set):
    return GlyphSet([ascii_set.glyph(ascii_set.find("STIX", "A")), ascii_set.glyph(ascii_set.find("STIX", "g"))])


def places_of(form):
    """glyph 0 ('A') at pens 40 and 58, glyph 1 ('g') between and over them"""
    if form == 0:
        return rg.make_places([(0, 64 * 40, 17), (1, 64 * 49 + 21, 12), (0, 64 * 58, 17)])
    if form == 1:
        return rg.make_places_ex([(0, 64 * 40, 64 * 17, 0.0, 0.25), (1, 64 * 49 + 21, 64 * 12 + 40, 0.0, 0.25),
                                  (0, 64 * 58, 64 * 17 + 13, 0.03, -0.5)])
    s = float(SCALE)
    c, sn = math.cos(math.radians(30.0)), math.sin(math.radians(30.0))
    return rg.make_places_affine([(0, 64 * 44, 64 * 18, 0.0, -s, s, 0.0), (1, 64 * 49 + 21, 64 * 12 + 40, s * c, -s * sn, s * sn, s * c),
                                  (0, 64 * 58, 64 * 17 + 13, s * c, s * sn, -s * sn, s * c)])


def runs():
    return rg.make_runs([RUN + (SCALE,)])


def mask_cells(form):
    """distinct (glyph, pen fractions, scale, slant) keys among the placements (all three survive clipping)"""
    pl = places_of(form)
    if form == 0:
        return len({(int(p["glyph"]), int(p["pen_x64"]) & 63) for p in pl})
    return len({(int(p["glyph"]), int(p["pen_x64"]) & 63, int(p["pen_y64"]) & 63, float(p["scale"]), float(p["slant"])) for p in pl})


def flags_of(k):
    return ((fr.FR_FILL_CONSISTENT if k.fill else 0) | (fr.FR_TEXT_SRGB if k.fam in (2, 4) else 0) | (fr.FR_TEXT_LOAD if k.fam in (3, 4) else 0)
            | (fr.FR_TEXT_OVER if k.blend == 2 else 0) | (fr.FR_TEXT_CACHE if k.cached else 0))


def start_buffer(k):
    """what the output holds before the render: the sentinel, or noise under FR_TEXT_LOAD"""
    if k.fam == 0:
        return np.full(SHAPE, SENT, np.uint8)
    if k.fam in (3, 4):
        return np.random.default_rng(11).integers(0, 256, SHAPE + (4,)).astype(np.uint8)
    return np.full(SHAPE + (4,), SENT, np.uint8)


def kernel_name(k):
    if k.cached:
        return f"fr::text_cached_kernel<{k.n}>" if k.fam == 0 else f"fr::text_cached_{FAMILIES[k.fam]}kernel<{k.n}, {k.blend}>"
    if k.fam == 0:
        return f"fr::text_{FORMS[k.form]}kernel<{k.n}, {k.fill}>"
    return f"fr::text_{FORMS[k.form]}{FAMILIES[k.fam]}kernel<{k.n}, {k.fill}, {k.blend}>"


def mask_name(k):
    return f"fr::glyph_mask_kernel<{k.n}, {k.fill}>"


def describe_of(k):
    """the whole fr_plan_describe string of the key's plan: two glyphs prepared, the mask cells of a cached plan, three instances"""
    parts = [f"fr::prepare_{'fill_' if k.fill else ''}kernel x2"]
    if k.cached:
        parts.append(f"{mask_name(k)} x{mask_cells(k.form)}")
    parts.append(f"{kernel_name(k)} x3")
    return "; ".join(parts)


def same_bytes_reason(a, b):
    """why two keys of one output format may render the same bytes, or None: with one sample per pixel and opaque colours
    every pixel is a placement's colour, the clear colour or the pixel that was there, which linear light returns
    unchanged (E(D[v]) = v), so FR_TEXT_SRGB changes no byte"""
    if a.n == 1 and a.blend == 0 and a.fam and b.fam and a._replace(fam=0) == b._replace(fam=0) and (a.fam in (3, 4)) == (b.fam in (3, 4)):
        return "N = 1 with opaque colours: every pixel is one colour exactly, and linear light returns it unchanged"
    return None

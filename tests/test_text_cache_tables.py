"""The FR_TEXT_CACHE tables of text plans (csrc/fr_text_plan.cpp: text_cache_tables) on the CPU: host/text_cache_selftest
runs the builder on a fixed list of small cases in both cacheable placement forms and checks by brute force what the
kernels of csrc/fr_text_cached.hip rely on: unique keys, every instance on the cell of exactly its own key, disjoint cell
extents whose sum is the reported total, every composite read of every pixel of every clipped cell inside the instance's
cell extent, every mask element stored exactly once, and the 2^31-element limit answered before a tile is listed.  It
prints one FNV-1a hash per case over the three tables; tests/golden/text_cache_tables.json holds those lines.  Also here:
the flag's value in the Python and Zig mirrors of the header."""
import json
import os
import re

import host_selftest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "text_cache_tables.json")


def _lines():
    return host_selftest.named("text_cache_selftest")


def test_text_cache_tables_match_golden():
    got = _lines()
    with open(GOLDEN) as f:
        want = json.load(f)
    assert list(got) == list(want), "the cases differ from the golden file's"
    wrong = {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    assert not wrong, wrong


def test_text_cache_tables_share_and_separate():
    """the counts the cases were built for: sharing where the key is equal, a cell of its own per differing key field"""
    got = _lines()
    count = {k: tuple(int(v) for v in re.search(r"insts (\d+) cells (\d+) tiles (\d+) elems (\d+)", line).groups())
             for k, line in got.items() if " error " not in " " + line}
    assert count["shared/plain"][:2] == (5, 3) and count["shared/ex"][:2] == (5, 3)
    assert count["no_sharing/plain"][:2] == (3, 3)
    assert count["one_field_each/ex"][:2] == (7, 6)            # glyph, fx, fy, scale, slant each split; the identical pair shares
    assert count["glyph_or_fraction/plain"][:2] == (4, 3)
    assert count["effective_scale/ex"][:2] == (4, 3)           # scale 0 is the run's; slant -0.0 is not slant 0.0
    assert count["three_runs/plain"][:2] == (6, 4)             # cells shared across the two runs of one scale
    assert count["clipped_away/plain"] == (0, 0, 0, 0)
    assert count["large_cell/plain"][2] == 60                  # 151 x 151 and 152 x 151 elements: 3 x 10 tiles each
    for form in ("plain", "ex"):
        assert got[f"err_store_cap/{form}"].startswith("error -4: FR_TEXT_CACHE: the mask cells hold more than 2^31 elements")


def test_flag_in_the_mirrors_of_the_header():
    import sys
    sys.path.insert(0, ROOT)
    import font_renderer_amd as fr
    from font_renderer_amd import _lib

    header = open(os.path.join(ROOT, "include", "fr_raster.h")).read()
    assert re.search(r"^#define FR_TEXT_CACHE 128u$", header, flags=re.M)
    assert _lib.FR_TEXT_CACHE == 128 and fr.FR_TEXT_CACHE == 128
    zig = open(os.path.join(ROOT, "bindings", "fr_raster.zig")).read()
    assert re.search(r"^pub const FR_TEXT_CACHE: u32 = 128;$", zig, flags=re.M)
    # the flag shares no bit with the others, and the unassigned bits stay unassigned
    others = _lib.FR_FILL_CONSISTENT | _lib.FR_TEXT_BGRA | _lib.FR_TEXT_SRGB | _lib.FR_TEXT_LOAD
    assert others & _lib.FR_TEXT_CACHE == 0 and (others | _lib.FR_TEXT_CACHE) & (2 | 16 | 64 | 1 << 31) == 0

"""The FR_TEXT_CACHE_AFFINE tables of matrix-form text plans (csrc/fr_text_plan.cpp: text_cache_tables for
fr_glyph_place_affine) on the CPU.  host/text_cache_affine_selftest runs the builder on a fixed list of small cases, checks by
brute force what glyph_mask_affine_kernel and the composites rely on (unique keys, every instance on the cell of its own key
with its own inverse matrix, back-to-back extents, every composite read inside its cell, every mask element stored once)
and prints the tables themselves.  tests/golden/text_cache_affine_tables.json holds the cases (glyph boxes, runs,
placements; the matrices as binary32 bit patterns) and the expected lines; the expected tables are made here, from a
restatement of the key, the cell (font_renderer_amd.text.instance_cell_affine), the clipping and the inverse of
include/fr_raster.h, not by the program under test: `python tests/test_text_cache_affine_tables.py` rewrites the lines of
the golden file from that restatement.  Also here: the flag's value in the mirrors of the header, and check_flags."""
import json
import os
import re
import struct
import sys

import numpy as np

import host_selftest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "text_cache_affine_tables.json")
CAP = 1 << 31
TILE_W, TILE_H = 64, 16


def _golden():
    with open(GOLDEN) as f:
        return json.load(f)


def _lines():
    return host_selftest.named("text_cache_affine_selftest")


def _f32(bits):
    return np.frombuffer(struct.pack("<I", bits), np.float32)[0]


def _bits(v):
    return struct.unpack("<I", struct.pack("<f", float(v)))[0]


def _inverse_bits(m):
    """include/fr_raster.h: D = xx*yy - xy*yx as two rounded binary64 products and one rounded difference; q00 = f32(yy / D),
    q01 = f32(-xy / D), q10 = f32(-yx / D), q11 = f32(xx / D) -> the four bit patterns"""
    xx, xy, yx, yy = (float(v) for v in m)
    a, b = xx * yy, xy * yx
    d = a - b
    return [_bits(np.float32(v)) for v in (yy / d, -xy / d, -yx / d, xx / d)]


def restate(gold, case):
    """the tables of one case -> the line the program must print after the case's name"""
    sys.path.insert(0, ROOT)
    from font_renderer_amd.text import instance_cell_affine

    boxes, seg = gold["boxes"], gold["seg_start"]
    cells, insts, cell_of_key, elems = [], [], {}, 0
    for first, count, w, h, _, _ in case["runs"]:
        if not w or not h:
            continue
        for g, px, py, mbits in case["places"][first:first + count]:
            if seg[g + 1] == seg[g]:
                continue                                               # no segment: no winding anywhere
            m = [_f32(b) for b in mbits]
            c0, r0, cw, ch = (int(v) for v in instance_cell_affine(boxes[g], m, px, py))
            x0, x1, y0, y1 = max(c0, 0), min(c0 + cw, w), max(r0, 0), min(r0 + ch, h)
            if x0 >= x1 or y0 >= y1:
                continue                                               # clipped away
            key = (g, px & 63, py & 63) + tuple(mbits)
            if key not in cell_of_key:
                if elems + cw * ch > CAP:
                    return "error -4: FR_TEXT_CACHE_AFFINE: the mask cells hold more than 2^31 elements; split the plan or drop the flag"
                cell_of_key[key] = len(cells)
                # the key's placement as an instance whose image is the whole cell: ix = -min_x, iy = max_y
                cells.append([g, px & 63, py & 63, (px >> 6) - c0, (py >> 6) - r0, cw, ch, 2 * seg[g], elems] + _inverse_bits(m))
                elems += cw * ch
            base = cells[cell_of_key[key]][8]
            insts.append((x0, x1, y0, y1, base, cw, c0, r0))
    tiles = [(k, x, y) for k, c in enumerate(cells) for y in range(0, c[6], TILE_H) for x in range(0, c[5], TILE_W)]
    if case.get("counts_only"):
        return "rc 0 insts %d cells %d elems %d" % (len(insts), len(cells), elems)
    return "insts %d cells %d tiles %d elems %d | C%s | I%s | T%s" % (
        len(insts), len(cells), len(tiles), elems,
        "".join(" " + ",".join(str(v) for v in c[:9]) + "," + ",".join("%08x" % q for q in c[9:]) + ";" for c in cells),
        "".join(" " + ",".join(str(v) for v in i) + ";" for i in insts),
        "".join(" %d,%d,%d;" % t for t in tiles))


def _parsed(line):
    """a table line -> (cells, composite records, tiles) as lists of lists of strings"""
    head, c, i, t = line.split(" | ")
    return [[r.split(",") for r in part[1:].replace(";", " ").split()] for part in (c, i, t)]


def test_tables_are_the_golden_file():
    got, gold = _lines(), _golden()
    assert list(got) == list(gold["lines"]), "the cases differ from the golden file's"
    wrong = {k: (got[k], gold["lines"][k]) for k in gold["lines"] if got[k] != gold["lines"][k]}
    assert not wrong, wrong


def test_golden_file_is_the_restatement():
    gold = _golden()
    assert [c["name"] for c in gold["cases"]] == [k for k in gold["lines"] if not k.startswith("launches/")]
    for case in gold["cases"]:
        assert gold["lines"][case["name"]] == restate(gold, case), case["name"]


def test_what_the_cases_were_built_for():
    got = _lines()
    count = {k: tuple(int(v) for v in re.match(r"insts (\d+) cells (\d+) tiles (\d+) elems (\d+)", line).groups())
             for k, line in got.items() if line.startswith("insts ")}
    # two placements of one key at different whole pens: one cell, two records with their own c0, r0 and the cell's pitch
    assert count["one_key_two_pens"][:2] == (2, 1)
    cells, insts, _ = _parsed(got["one_key_two_pens"])
    assert [i[4:] for i in insts] == [["0", "11", "6", "7"], ["0", "11", "13", "9"]] and cells[0][5:7] == ["11", "17"]
    assert count["two_matrices"][:2] == (3, 2)                         # one glyph under two matrices; the third shares the first's
    assert count["signed_zero"][:2] == (2, 2)                          # 0.0 and -0.0 are two keys
    cells, _, _ = _parsed(got["signed_zero"])
    assert cells[0][:9] == cells[1][:8] + ["0"] and cells[0][10] == "80000000" and cells[1][10] == "00000000"
    # neither fraction, fx only, fy only, both (twice): cw and ch grow by one with their fraction
    assert count["fractions"][:2] == (5, 4)
    cells, _, _ = _parsed(got["fractions"])
    assert [(c[1], c[2], c[5], c[6]) for c in cells] == [("0", "0", "7", "9"), ("8", "0", "8", "9"), ("0", "8", "7", "10"), ("8", "8", "8", "10")]
    assert count["quarter_mirror_turn"][:2] == (4, 3)                  # the quarter turn twice
    # half outside the run: the cell is whole, the record clipped
    cells, insts, _ = _parsed(got["half_outside"])
    assert len(cells) == 1 and cells[0][5:7] == ["11", "17"]
    assert insts[0][:4] == ["36", "40", "20", "30"] and insts[1][:4] == ["0", "7", "0", "6"] and insts[1][6:] == ["-4", "-11"]
    assert count["skipped_between"][:2] == (2, 1)                      # the survivors on either side of three that are not
    assert count["no_segments"] == count["clipped_away"] == count["no_runs"] == (0, 0, 0, 0)
    cells, _, tiles = _parsed(got["tiles"])
    assert [(c[5], c[6]) for c in cells] == [("1", "1"), ("64", "16"), ("65", "17"), ("65", "16"), ("64", "17"), ("2", "2")]
    assert [sum(1 for t in tiles if int(t[0]) == k) for k in range(6)] == [1, 1, 4, 2, 2, 1]
    assert count["two_runs"][:2] == (4, 3)
    assert got["err_store_cap"].startswith("error -4: FR_TEXT_CACHE_AFFINE: the mask cells hold more than 2^31 elements")
    # one of the two cells alone is within the limit, so the limit is the sum's
    assert got["one_huge_cell"] == "rc 0 insts 2 cells 1 elems %d" % (40001 * 40001) and 40001 * 40001 < CAP < 2 * 40001 * 40001


def test_launch_lists():
    got = _lines()
    assert got["launches/affine"] == "prepare fr::prepare_kernel x1; mask fr::glyph_mask_affine_kernel<4, 0> x1; cached fr::text_cached_kernel<4> x1"
    for form in ("ex", "plain"):
        assert got["launches/" + form] == "prepare fr::prepare_kernel x1; mask fr::glyph_mask_kernel<4, 0> x1; cached fr::text_cached_kernel<4> x1"


def test_flag_in_the_mirrors_of_the_header():
    sys.path.insert(0, ROOT)
    import font_renderer_amd as fr
    from font_renderer_amd import _lib

    header = open(os.path.join(ROOT, "include", "fr_raster.h")).read()
    assert re.search(r"^#define FR_TEXT_CACHE_AFFINE 512u$", header, flags=re.M)
    assert _lib.FR_TEXT_CACHE_AFFINE == 512 and fr.FR_TEXT_CACHE_AFFINE == 512
    zig = open(os.path.join(ROOT, "bindings", "fr_raster.zig")).read()
    assert re.search(r"^pub const FR_TEXT_CACHE_AFFINE: u32 = 512;$", zig, flags=re.M)
    # the flag shares no bit with the others, and the unassigned bits stay unassigned
    others = (_lib.FR_FILL_CONSISTENT | _lib.FR_TEXT_BGRA | _lib.FR_TEXT_SRGB | _lib.FR_TEXT_LOAD | _lib.FR_TEXT_CACHE | _lib.FR_TEXT_OVER)
    assert others == 1 | 4 | 8 | 32 | 128 | 256
    assert others & _lib.FR_TEXT_CACHE_AFFINE == 0 and (others | _lib.FR_TEXT_CACHE_AFFINE) & (2 | 16 | 64 | 1 << 31) == 0
    # every flag the header defines for this flag word is one of those
    words = {name: int(v) for name, v in re.findall(r"^#define (FR_FILL_CONSISTENT|FR_TEXT_[A-Z_]+) (\d+)u$", header, flags=re.M)}
    assert sum(words.values()) == others | 512 and len(words) == 7, words


def test_check_flags_refuses_it_unless_allowed():
    """host/text_cache_affine_flags_selftest: check_flags takes 512 only where it is passed as allowed; the two _affine entry
    points pass it (csrc/fr_api_plan.hip), and no other unit names it"""
    got = host_selftest.named("text_cache_affine_flags_selftest")
    ok = {k for k, v in got.items() if v == "rc=0 ok"}
    assert ok == {"affine", "affine-fill", "affine-rgba-all"}, got
    assert got["raster"] == got["upright"] == got["upright-rgba"] == "rc=-1 err=unknown flag bits 0x200"
    assert got["both-caches-affine"] == "rc=-1 err=unknown flag bits 0x80" and got["both-caches-upright"] == "rc=-1 err=unknown flag bits 0x200"
    assert got["affine-coverage-srgb"] == "rc=-1 err=unknown flag bits 0x8"
    assert [got[k] for k in ("bit1", "bit4", "bit6", "top")] == ["rc=-1 err=unknown flag bits 0x%x" % b for b in (2, 16, 64, 1 << 31)]
    glue = open(os.path.join(ROOT, "font-renderer_amd", "csrc", "fr_api_plan.hip")).read()
    assert glue.count("FR_TEXT_CACHE_AFFINE : FR_TEXT_CACHE;") == 1
    for unit in ("fr_api_glyph.hip", "fr_api_layer.hip", "fr_api_exact.hip", "fr_api_ctx.hip", "fr_host_rules.cpp"):
        assert "FR_TEXT_CACHE_AFFINE" not in open(os.path.join(ROOT, "font-renderer_amd", "csrc", unit)).read(), unit


if __name__ == "__main__":
    gold = _golden()
    for case in gold["cases"]:
        gold["lines"][case["name"]] = restate(gold, case)
    with open(GOLDEN, "w") as f:
        json.dump(gold, f, indent=1)
        f.write("\n")

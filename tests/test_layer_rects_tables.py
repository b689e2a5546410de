"""The host side of fr_layer_rects (csrc/fr_layer_rects_plan.cpp) on the CPU: host/layer_rects_selftest prints, for each
case, the inputs and what the builder made of them: the records, the tiles and the index list, or the refusal.  Every line
is compared with a restatement of the checks, the clipping and the binning written here from include/fr_raster.h and the
comments of fr_layer_rects_plan.hpp, computed from the inputs the line itself names; the program checks the properties of
its tables on its own and fails if one does not hold."""
import host_selftest
import layer_rects_ref as rr

TILE_W, TILE_H, MAX_EDGE, MAX_TILES, MAX_PAIRS = 256, 16, 2 ** 31 - 1, 1 << 22, 1 << 24


def _lines():
    return host_selftest.cases("layer_rects_selftest")


def _rows(text):
    return [] if text == "-" else [tuple(int(v) for v in r.split(",")) for r in text.split(";")]


def _clipped(inp):
    """the records: (x0, y0, x1, y1, rgba, index) of every rectangle that draws"""
    _, ds, dr, _ = (int(v) for v in inp["in"].split(","))
    w64, h64 = min(64 * ds, MAX_EDGE), min(64 * dr, MAX_EDGE)
    recs = []
    for j, (x0, y0, x1, y1, r, g, b, a) in enumerate(_rows(inp["rects"])):
        x0, x1, y0, y1 = (min(max(v, 0), lim) for v, lim in ((x0, w64), (x1, w64), (y0, h64), (y1, h64)))
        if x0 < x1 and y0 < y1 and a:
            recs.append((x0, y0, x1, y1, r | g << 8 | b << 16 | a << 24, j))
    return recs


def _tile_ranges(rec):
    x0, y0, x1, y1 = rec[:4]
    return range(x0 // (64 * TILE_W), (x1 - 1) // (64 * TILE_W) + 1), range(y0 // (64 * TILE_H), (y1 - 1) // (64 * TILE_H) + 1)


def _expect(inp, null_rects):
    """the restatement: (rc, None) or (0, (vec, recs, tiles, list))"""
    dst, ds, dr, flags = (int(v) for v in inp["in"].split(","))
    if flags & ~1:
        return -1, None
    if dst == 0 or dst % 4 or ds > 1 << 26:
        return -1, None
    if dr >= 1 << 31:
        return -4, None
    if _rows(inp["rects"]) and null_rects:
        return -1, None
    recs = _clipped(inp)
    sizes = [len(tx) * len(ty) for tx, ty in map(_tile_ranges, recs)]
    if max(sizes, default=0) > MAX_TILES or sum(sizes) > MAX_PAIRS:
        return -4, None
    # distinct tiles, counted row by row as the union of the rectangles' column ranges
    spans = {}
    for rec in recs:
        tx, ty = _tile_ranges(rec)
        for y in ty:
            spans.setdefault(y, []).append((tx.start, tx.stop))
    distinct = 0
    for row in spans.values():
        end = 0
        for lo, hi in sorted(row):
            distinct += max(0, hi - max(lo, end))
            end = max(end, hi)
    if distinct > MAX_TILES:
        return -4, None
    tiles = {}
    for k, rec in enumerate(recs):
        tx, ty = _tile_ranges(rec)
        for y in ty:
            for x in tx:
                tiles.setdefault((y, x), []).append(k)
    assert len(tiles) == distinct
    table, lst = [], []
    for (y, x) in sorted(tiles):
        table.append((x * TILE_W, y * TILE_H, len(lst), len(tiles[(y, x)])))
        lst += tiles[(y, x)]
    return 0, (int(dst % 16 == 0 and ds % 4 == 0), recs, table, [(i,) for i in lst])


def _tables(tail):
    got = dict(f.split("=", 1) for f in tail.split(" "))
    return int(got["vec"]), _rows(got["recs"]), _rows(got["tiles"]), _rows(got["list"])


def test_every_line_matches_the_restatement():
    lines = _lines()
    assert len(lines) >= 35
    for name, (inp, null_rects, tail) in lines.items():
        rc, want = _expect(inp, null_rects)
        assert int(inp["rc"]) == rc, (name, inp["rc"], rc, tail)
        if rc:
            assert tail.startswith("err=") and len(tail) > 4, (name, tail)
            continue
        assert _tables(tail) == want, name


def test_lists_ascend_and_no_tile_lies_outside_a_bounding_box():
    seen = 0
    for name, (inp, _, tail) in _lines().items():
        if int(inp["rc"]):
            continue
        _, ds, dr, _ = (int(v) for v in inp["in"].split(","))
        _, recs, tiles, lst = _tables(tail)
        rects = _rows(inp["rects"])
        for x, y, first, count in tiles:
            mine = [lst[first + i][0] for i in range(count)]
            assert mine == sorted(set(mine)), (name, x, y)
            assert [recs[k][5] for k in mine] == sorted(recs[k][5] for k in mine), (name, x, y)      # the caller's order
            for k in mine:                                  # the caller's rectangle, by the twin's bounding box, meets the tile
                box = rr.bounding_box(rects[recs[k][5]], min(ds, 1 << 25), min(dr, 1 << 25))
                assert box and box[0] < x + TILE_W and box[2] > x and box[1] < y + TILE_H and box[3] > y, (name, x, y, k)
            seen += count
    assert seen > 200                                       # (the long list of many_in_one_tile alone)


def test_the_named_cases():
    L = _lines()
    rc = {k: int(v[0]["rc"]) for k, v in L.items()}
    T = {k: _tables(v[2]) for k, v in L.items() if rc[k] == 0}
    for k in ("far_outside", "inverted", "all_transparent", "no_rects"):
        assert rc[k] == 0 and T[k][1:] == ([], [], []), k
    assert T["extreme_edges"][1] == [(0, 0, 132 * 64, 50 * 64, 10 | 20 << 8 | 30 << 16 | 255 << 24, 0)] and len(T["extreme_edges"][2]) == 4
    assert [r[5] for r in T["transparent_dropped"][1]] == [1]
    assert len(T["tile_row_border"][2]) == 2 and len(T["ends_on_tile_row_border"][2]) == 1
    assert [t[:2] for t in T["tile_column_border"][2]] == [(0, 0), (256, 0), (512, 0), (256, 16), (512, 16)] and len(T["ends_on_tile_column_border"][2]) == 1
    assert T["whole_image"][0] == 1 and T["rows131_no_vec"][0] == 0 and T["dst_4_aligned_only"][0] == 0
    assert len(T["many_in_one_tile"][1]) > 200 and T["many_in_one_tile"][2][0][3] > 200           # one long list
    assert T["pitch_max"][2] == [((1 << 25) - 256, 0, 0, 1)] and T["tall_image_last_reachable_rows"][2] == [(0, (1 << 25) - 16, 0, 1)]
    # every refusal, and the order of the checks: one case per rule, the earlier rule's code
    assert rc["unknown_flag_2"] == -1 and rc["text_flag_bits"] == -1 and rc["dst_null"] == -1 and rc["dst_not_4_aligned"] == -1
    assert rc["pitch_over"] == -1 and rc["rows_over"] == -4 and rc["rects_null"] == -1
    assert rc["order_flag_before_dst"] == -1 and "flag" in L["order_flag_before_dst"][2]
    assert rc["order_dst_before_pitch"] == -1 and "aligned" in L["order_dst_before_pitch"][2]
    assert rc["order_pitch_before_rows"] == -1 and rc["order_rows_before_null_rects"] == -4 and rc["order_null_rects_before_limits"] == -1
    # both limits
    assert rc["tiles_over_one_rect"] == -4 and "tiles" in L["tiles_over_one_rect"][2]
    assert rc["tiles_over_two_rects"] == -4 and "tiles" in L["tiles_over_two_rects"][2]
    assert rc["tiles_at_limit_pairs_over"] == -4 and "pairs" in L["tiles_at_limit_pairs_over"][2]

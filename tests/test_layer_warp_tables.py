"""The host side of fr_layer_warp (csrc/fr_layer_warp_plan.cpp) on the CPU: host/layer_warp_selftest prints, for each case,
the inputs and what the builder made of them: the clipped rectangles and the tile table, or the refusal.  Every line is
compared with a restatement of the checks in the header's order, the clipping, the overlap rule, the culling of the tiles no
tap can reach, the tiles' origins and tap boxes and the vector flag, written here from include/fr_raster.h and the comments
of fr_layer_warp_plan.hpp and computed from the inputs the line itself names; the program checks the properties of its
tables pixel by pixel on its own and fails if one does not hold.  There is one access path, the gather, so no path is
chosen per tile; the two things a tile does choose, the vector flag and the opacity instance, are checked."""
import ctypes as C

import numpy as np

import font_renderer_amd as fr
import host_selftest
from font_renderer_amd import _lib

TILE, LANE_PX, DST_VEC = 32, 4, 0x100
ONE, HALF = 65536, 32768
INVALID, UNSUPPORTED = -1, -4


def _lines():
    return host_selftest.cases("layer_warp_selftest")


def _rows(text):
    return [] if text == "-" else [tuple(int(v) for v in r.split(",")) for r in text.split(";")]


def _extremes(u, ux, uy, X0, X1, Y0, Y1):
    """an affine function over a box: its extremes sit at the corners (arrays of boxes that broadcast)"""
    corners = [u + X * ux + Y * uy for X in (X0, X1) for Y in (Y0, Y1)]
    return np.minimum.reduce(corners), np.maximum.reduce(corners)


def _expect(inp, null_blits):
    """the restatement: (rc, None) or (0, (pixels, walked, opacity, clips, tiles))"""
    src, dst, ss, sr, ds, dr, flags = (int(v) for v in inp["in"].split(","))
    blits = _rows(inp["blits"])
    if flags & ~1:
        return INVALID, None
    if src == 0 or src % 4 or ss > 1 << 26:
        return INVALID, None
    if dst == 0 or dst % 4 or ds > 1 << 26:
        return INVALID, None
    if sr >= 1 << 31 or dr >= 1 << 31:
        return UNSUPPORTED, None
    if blits and null_blits:
        return INVALID, None
    if src < dst + 4 * ds * dr and dst < src + 4 * ss * sr:
        return INVALID, None
    clips, walked, pixels = [], 0, 0
    for sx, sy, w, h, dx, dy, dw, dh, u0, v0, ux, uy, vx, vy, o, reserved in blits:
        if o > 255 or reserved:
            return INVALID, None
        if abs(u0) > 1 << 47 or abs(v0) > 1 << 47:
            return INVALID, None
        if dw > 1 << 26 or dh > 1 << 26:
            return INVALID, None
        if sx + w > ss or sy + h > sr:
            return INVALID, None
        x0, y0, x1, y1 = max(dx, 0), max(dy, 0), min(dx + dw, ds), min(dy + dh, dr)
        if dw == 0 or dh == 0 or x0 >= x1 or y0 >= y1:
            clips.append(None)
            continue
        clips.append((x0, y0, x1, y1, x0 - dx, y0 - dy))
        pixels += (x1 - x0) * (y1 - y0)
        if o and w and h:
            walked += -(-(x1 - x0 // LANE_PX * LANE_PX) // TILE) * -(-(y1 - y0) // TILE)
    if walked > 1 << 22:
        return UNSUPPORTED, None
    for i, a in enumerate(clips):
        for b in clips[i + 1:]:
            if a and b and a[0] < b[2] and b[0] < a[2] and a[1] < b[3] and b[1] < a[3]:
                return INVALID, None
    dvec = dst % 16 == 0 and ds % 4 == 0
    tiles, opacity = [], 0
    for c, (sx, sy, w, h, dx, dy, dw, dh, u0, v0, ux, uy, vx, vy, o, _) in zip(clips, blits):
        if c is None or o == 0 or w == 0 or h == 0:
            continue
        x0, y0, x1, y1 = c[:4]
        before = len(tiles)
        # every tile of the clipped rectangle at once (int64 throughout: |U| stays below 2^59)
        xs, ys = np.arange(x0 // LANE_PX * LANE_PX, x1, TILE, dtype=np.int64)[None, :], np.arange(y0, y1, TILE, dtype=np.int64)[:, None]
        X0, X1, Y0, Y1 = np.maximum(xs, x0) - dx, np.minimum(xs + TILE, x1) - 1 - dx, ys - dy, np.minimum(ys + TILE, y1) - 1 - dy
        (ulo, uhi), (vlo, vhi) = _extremes(u0, ux, uy, X0, X1, Y0, Y1), _extremes(v0, vx, vy, X0, X1, Y0, Y1)
        # a pixel at U has the tap columns (U - HALF) >> 16 and the next; column i is in the window for 0 <= i < w
        i_lo, i_hi, j_lo, j_hi = (ulo - HALF) >> 16, ((uhi - HALF) >> 16) + 1, (vlo - HALF) >> 16, ((vhi - HALF) >> 16) + 1
        keep = (i_hi >= 0) & (i_lo <= w - 1) & (j_hi >= 0) & (j_lo <= h - 1)
        for r, k in np.argwhere(keep).tolist():                 # rows of tiles top to bottom, left to right
            x, y = int(xs[0, k]), int(ys[r, 0])
            tiles.append((x, y, x0, x1, y1, o | (DST_VEC if dvec else 0), sx, sy, u0 + (x - dx) * ux + (y - dy) * uy, v0 + (x - dx) * vx + (y - dy) * vy, ux, uy, vx, vy,
                          w, h, max(int(i_lo[r, k]), 0), max(int(j_lo[r, k]), 0), min(int(i_hi[r, k]), w - 1), min(int(j_hi[r, k]), h - 1)))
        if len(tiles) > before and o != 255:
            opacity = 1
    return 0, (pixels, walked, opacity, [c or (0, 0, 0, 0, 0, 0) for c in clips], tiles)


def _tail(tail):
    return dict(f.split("=", 1) for f in tail.split(" "))


def test_every_line_matches_the_restatement():
    lines = _lines()
    assert len(lines) >= 95
    for name, (inp, null_blits, tail) in lines.items():
        rc, want = _expect(inp, null_blits)
        assert int(inp["rc"]) == rc, (name, inp["rc"], rc, tail)
        if rc:
            assert tail.startswith("err=") and len(tail) > 4, (name, tail)
            continue
        got = _tail(tail)
        assert (int(got["pixels"]), int(got["walked"]), int(got["opacity"]), _rows(got["clips"]), _rows(got["tiles"])) == want, name


def test_the_named_cases():
    L = _lines()
    rc = {k: int(v[0]["rc"]) for k, v in L.items()}
    err = {k: v[2][4:] for k, v in L.items() if rc[k]}
    tails = {k: _tail(v[2]) for k, v in L.items() if rc[k] == 0}
    tiles = {k: _rows(t["tiles"]) for k, t in tails.items()}
    # the checks in order, every refusal with its code
    for k in ("unknown_flag_2", "unknown_flag_4", "unknown_flag_8", "unknown_flag_16", "unknown_flag_256", "unknown_flag_2147483648", "flag_comes_before_src"):
        assert rc[k] == INVALID and "flag" in err[k], k
    for k in ("src_null", "src_not_4_aligned", "src_pitch_over", "src_comes_before_dst"):
        assert rc[k] == INVALID and err[k].startswith("src"), (k, err[k])
    for k in ("dst_null", "dst_not_4_aligned", "dst_pitch_over", "dst_comes_before_rows"):
        assert rc[k] == INVALID and err[k].startswith("dst"), (k, err[k])
    for k in ("dst_rows_over", "src_rows_over", "rows_come_before_blits"):
        assert rc[k] == UNSUPPORTED and "rows" in err[k], (k, err[k])
    for k in ("blits_null", "blits_come_before_aliasing"):
        assert rc[k] == INVALID and "blits is NULL" in err[k], (k, err[k])
    for k in ("aliasing_comes_before_opacity", "dst_in_the_layers_last_pixel"):
        assert rc[k] == INVALID and "overlap in memory" in err[k], (k, err[k])
    assert rc["dst_behind_the_layer"] == 0
    for k in ("opacity_256", "opacity_comes_before_reserved"):
        assert rc[k] == INVALID and "opacity" in err[k], (k, err[k])
    for k in ("reserved_1", "reserved_1_on_an_empty_blit", "reserved_comes_before_origin"):
        assert rc[k] == INVALID and "reserved" in err[k], (k, err[k])
    for k in ("origin_over", "origin_v_under", "origin_comes_before_rectangle"):
        assert rc[k] == INVALID and "2^47" in err[k], (k, err[k])
    for k in ("rectangle_width_over", "rectangle_height_over", "rectangle_comes_before_window"):
        assert rc[k] == INVALID and "2^26" in err[k], (k, err[k])
    for k in ("window_one_pixel_out_right", "window_one_row_out_below", "zero_width_window_out_of_the_layer", "window_comes_before_overlap"):
        assert rc[k] == INVALID and "leaves the layer" in err[k], (k, err[k])
    assert rc["window_last_column_in"] == 0 and rc["pitch_max"] == 0 and rc["tall_image_last_rows"] == 0 and rc["rectangle_max"] == 0
    assert rc["too_many_tiles"] == UNSUPPORTED and "tiles" in err["too_many_tiles"]
    assert rc["as_many_tiles_as_allowed"] == 0 and int(tails["as_many_tiles_as_allowed"]["walked"]) == 1 << 22
    assert rc["too_many_tiles_counts_no_opacity_0_blit"] == 0 and tiles["too_many_tiles_counts_no_opacity_0_blit"] == []
    # the overlap rule: every clipped rectangle counts, whether it draws or not; the message names the first pair
    for k in ("two_overlap_by_one_pixel", "overlap_with_an_opacity_0_blit", "overlap_with_a_blit_no_tap_reaches"):
        assert rc[k] == INVALID and "overlap in the destination" in err[k], (k, err[k])
    assert rc["overlap_only_before_clipping"] == 0 and "blits 1 and 2" in err["overlap_names_the_first_pair"]
    # valid calls that list no tile, and so launch nothing
    for k in ("no_tap_reaches_the_window", "first_tap_that_misses_on_the_left", "wholly_off_the_image", "wholly_off_the_image_by_min", "far_right_max",
              "zero_matrix_outside_the_window", "coefficients_max_over_the_largest_rectangle", "origin_minus_2_47_far_away",
              "zero_width_rectangle", "zero_width_window", "all_opacity_0", "no_blits"):
        assert rc[k] == 0 and tiles[k] == [], k
    # the culling: which tiles of a large rectangle around a small window are listed
    assert [t[:2] for t in tiles["small_window_in_the_whole_image"]] == [(96, 64), (96, 96)]          # the window's pixels at 100 .. 107, 90 .. 97; taps one more
    assert [t[:2] for t in tiles["huge_rectangle_around_a_small_window"]] == [(128, 96)]               # at 150 .. 157, 100 .. 107
    assert int(tails["huge_rectangle_around_a_small_window"]["walked"]) == 10 * 7 and int(tails["huge_rectangle_around_a_small_window"]["pixels"]) == 300 * 200
    assert tiles["huge_rectangle_around_a_small_window"][0][16:] == (0, 0, 7, 7)
    assert [t[:2] for t in tiles["last_tap_column_reaches_the_window"]] == [(0, 0), (0, 32)]           # column 0 alone, rows 0 .. 50
    assert [t[16:] for t in tiles["last_tap_column_reaches_the_window"]] == [(69, 0, 69, 32), (69, 32, 69, 49)]
    assert len(tiles["last_tap_that_hits_on_the_left"]) == 1 and tiles["last_tap_that_hits_on_the_left"][0][16:] == (0, 0, 0, 1)
    assert len(tiles["zero_matrix_in_the_window"]) == 4 and all(t[16:] == (4, 5, 5, 6) and t[8:10] == (5 * ONE + 77, 6 * ONE + 99) for t in tiles["zero_matrix_in_the_window"])
    assert [t[:2] for t in tiles["coefficients_max"]] == [(0, 0)] and [t[:2] for t in tiles["coefficients_min_plus_one"]] == [t[:2] for t in tiles["coefficients_int32_min"]] == [(0, 0)]
    assert [t[:2] for t in tiles["origin_plus_2_47"]] == []                                            # 2^47 / (2^31 - 1) is beyond column 300
    assert [t[:2] for t in tiles["origin_minus_2_47_walks_into_the_window"]] == [(131072, 0)] and tiles["origin_minus_2_47_walks_into_the_window"][0][8] == 0
    assert 0 < len(tiles["turned_45"]) < 16 and len(tiles["identity_whole_layer"]) == 6
    assert len(tiles["rectangle_one_larger_all_round"]) == 6 and tiles["rectangle_one_larger_all_round"][0][:5] == (8, 9, 9, 81, 61)
    # a tile's origin: x is rounded down to the lane's four pixels and U follows it below the rectangle's edge
    t = tiles["identity_negative_offsets"][0]
    assert t[:5] == (0, 0, 0, 65, 43) and t[8:10] == (HALF + 5 * ONE, HALF + 7 * ONE)
    for dx in range(4):
        t = tiles[f"dst_x_{dx}_across_a_tile_border"]
        assert [x[:2] for x in t] == [(28, 25), (60, 25)] and t[0][8] == HALF - dx * ONE and t[0][6:8] == (9, 11) and t[0][14:16] == (37, 21)
    # several blits: blit by blit; the opacity and the maps per tile; the OPACITY instance only where a listed tile needs it
    assert sorted({t[5] & 255 for t in tiles["touching_rectangles_with_their_own_maps"]}) == [1, 77, 128, 255]
    assert [t[5] & 255 for t in tiles["touching_rectangles_with_their_own_maps"]] == sorted((t[5] & 255 for t in tiles["touching_rectangles_with_their_own_maps"]),
                                                                                             key=[255, 128, 1, 77].index)
    assert tails["touching_rectangles_with_their_own_maps"]["opacity"] == "1" and tails["identity_whole_layer"]["opacity"] == "0"
    assert tails["opacity_instance_only_for_listed_tiles"]["opacity"] == "0" and len(tiles["opacity_0_has_no_tile"]) == 6
    assert tails["turned_45_srgb_opacity"]["opacity"] == "1"
    # the shapes of tests/test_gpu_layer_warp.py reach both kinds of group: whole groups of a vector tile, and tiles without the flag
    flags = {k: {t[5] & ~255 for t in v} for k, v in tiles.items() if v}
    assert flags["identity_whole_layer"] == {DST_VEC} and flags["dst_4_aligned_only"] == {0} and flags["dst_rows_off_the_grid"] == {0}
    assert flags["src_4_aligned_only_and_odd_pitch"] == {DST_VEC}                                      # the layer's grid does not matter: it is gathered
    assert len(tiles["windows_1x1_1x9_9x1"]) == 3


def test_the_blit_struct():
    """fr_layer_warp_blit as the ctypes structure and as the numpy row make_warp_blits builds"""
    row = (1, 2, 30, 40, -5, -6, 70, 80, -(1 << 47), (1 << 47), -(1 << 31), (1 << 31) - 1, 65536, -65536, 200)
    table = fr.make_warp_blits([row])
    assert table.shape == (1,) and table.dtype.itemsize == C.sizeof(_lib.LayerWarpBlit) == 72
    raw = _lib.LayerWarpBlit.from_buffer_copy(table.tobytes())
    assert tuple(getattr(raw, n) for n, _ in _lib.LayerWarpBlit._fields_) == row + (0,)
    assert np.dtype(_lib.LayerWarpBlit).names == ("src_x", "src_y", "w", "h", "dst_x", "dst_y", "dst_w", "dst_h", "u0", "v0", "ux", "uy", "vx", "vy", "opacity", "reserved")
    assert fr.make_warp_blits([row + (7,)])["reserved"][0] == 7

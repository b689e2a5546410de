"""The host side of fr_layer_mask (csrc/fr_layer_mask_plan.cpp) on the CPU: host/layer_mask_selftest prints, for each case,
the inputs and what the builder made of them: the clipped rectangles, the mask origins and the tile table, or the refusal.
Every line is compared with a restatement of the checks in the header's order, the clipping, the overlap rule, the three
vector flags and the tiling, written here from include/fr_raster.h and the comments of fr_layer_mask_plan.hpp and computed
from the inputs the line itself names; the program checks the coverage properties of its tables on its own and fails if
one does not hold."""
import ctypes as C

import numpy as np

import font_renderer_amd as fr
import host_selftest
import layer_ref as lr
from font_renderer_amd import _lib

TILE_W, TILE_H, LANE_PX, DST_VEC, SRC_VEC, MASK_VEC = 256, 16, 4, 0x100, 0x200, 0x400
SRGB, PLANE, ERASE = 1, 4, 8
INVALID, UNSUPPORTED = -1, -4


def _lines():
    return host_selftest.cases("layer_mask_selftest")


def _rows(text):
    return [] if text == "-" else [tuple(int(v) for v in r.split(",")) for r in text.split(";")]


def _expect(inp, null_blits):
    """the restatement: (rc, None) or (0, (pixels, clips, origins, tiles))"""
    src, mask, dst, ss, sr, ms, mr, ds, dr, flags = (int(v) for v in inp["in"].split(","))
    blits = _rows(inp["blits"])
    plane, erase = bool(flags & PLANE), bool(flags & ERASE)
    if flags & ~(SRGB | PLANE | ERASE):
        return INVALID, None
    if dst == 0 or dst % 4 or ds > 1 << 26:
        return INVALID, None
    if mask == 0 or ms > 1 << 26 or (not plane and mask % 4):
        return INVALID, None
    if erase != (src == 0):
        return INVALID, None
    if not erase and (src % 4 or ss > 1 << 26):
        return INVALID, None
    if (not erase and sr >= 1 << 31) or mr >= 1 << 31 or dr >= 1 << 31:
        return UNSUPPORTED, None
    if blits and null_blits:
        return INVALID, None
    msize = ms * mr * (1 if plane else 4)
    if not erase and src < dst + 4 * ds * dr and dst < src + 4 * ss * sr:
        return INVALID, None
    if mask < dst + 4 * ds * dr and dst < mask + msize:
        return INVALID, None
    clips, origins = [], []
    for sx, sy, w, h, dx, dy, mx, my, o, inv in blits:
        if o > 255 or inv > 1:
            return INVALID, None
        if w and h and not erase and (sx + w > ss or sy + h > sr):
            return INVALID, None
        if w and h and (mx + w > ms or my + h > mr):
            return INVALID, None
        if erase:
            sx = sy = 0
        c = lr.clip((sx, sy, w, h, dx, dy, o), ds, dr)
        clips.append(c)
        origins.append((mx + c[4] - sx, my + c[5] - sy) if c else (0, 0))
    n_tiles = sum(-(-(c[2] - c[0] // LANE_PX * LANE_PX) // TILE_W) * -(-(c[3] - c[1]) // TILE_H) for c, b in zip(clips, blits) if c and b[8])
    if n_tiles > 1 << 22:
        return UNSUPPORTED, None
    for i, a in enumerate(clips):
        for b in clips[i + 1:]:
            if a and b and a[0] < b[2] and b[0] < a[2] and a[1] < b[3] and b[1] < a[3]:
                return INVALID, None
    dvec = dst % 16 == 0 and ds % 4 == 0
    svec = not erase and src % 16 == 0 and ss % 4 == 0
    tiles, pixels = [], 0
    for c, g, b in zip(clips, origins, blits):
        if c is None:
            continue
        x0, y0, x1, y1, sx, sy = c
        pixels += (x1 - x0) * (y1 - y0)
        o, inv = b[8], b[9]
        if o == 0:
            continue
        tx0 = x0 - x0 % LANE_PX
        sx0, mx0 = sx - (x0 - tx0), g[0] - (x0 - tx0)
        # a layer mask: the group on the mask's 16-byte grid; a plane: its four bytes on a 4-byte grid, pointer + pitch + column
        mvec = ms % 4 == 0 and ((mask + mx0) % 4 == 0 if plane else mask % 16 == 0 and mx0 % 4 == 0)
        ov = o | (DST_VEC if dvec else 0) | (SRC_VEC if svec and sx0 % LANE_PX == 0 else 0) | (MASK_VEC if mvec else 0)
        for y in range(y0, y1, TILE_H):
            for x in range(tx0, x1, TILE_W):
                tiles.append((x, y, x0, x1, y1, sx0 + x - tx0, sy + y - y0, ov, mx0 + x - tx0, g[1] + y - y0, inv))
    return 0, (pixels, [c or (0, 0, 0, 0, 0, 0) for c in clips], origins, tiles)


def _tail(tail):
    return dict(f.split("=", 1) for f in tail.split(" "))


def test_every_line_matches_the_restatement():
    lines = _lines()
    assert len(lines) >= 100
    for name, (inp, null_blits, tail) in lines.items():
        rc, want = _expect(inp, null_blits)
        assert int(inp["rc"]) == rc, (name, inp["rc"], rc, tail)
        if rc:
            assert tail.startswith("err=") and len(tail) > 4, (name, tail)
            continue
        got = _tail(tail)
        assert (int(got["pixels"]), _rows(got["clips"]), _rows(got["origins"]), _rows(got["tiles"])) == want, name


def test_the_named_cases():
    L = _lines()
    rc = {k: int(v[0]["rc"]) for k, v in L.items()}
    err = {k: v[2][4:] for k, v in L.items() if rc[k]}
    tiles = {k: _rows(_tail(v[2])["tiles"]) for k, v in L.items() if rc[k] == 0}
    # the checks in order, every refusal with its code
    for k in ("unknown_flag_lcd_bgr", "unknown_flag_16", "text_flag_bits", "flag_comes_before_dst"):
        assert rc[k] == INVALID and "flag" in err[k], k
    for k in ("dst_null", "dst_not_4_aligned", "dst_pitch_over", "dst_comes_before_mask"):
        assert rc[k] == INVALID and err[k].startswith("dst"), (k, err[k])
    for k in ("mask_null", "plane_null", "mask_not_4_aligned", "mask_pitch_over", "plane_pitch_over", "mask_comes_before_src", "mask_comes_before_erase_src"):
        assert rc[k] == INVALID and err[k].startswith("mask"), (k, err[k])
    for k in ("src_null", "erase_with_a_src", "erase_with_a_misaligned_src", "src_not_4_aligned", "src_pitch_over", "src_comes_before_rows"):
        assert rc[k] == INVALID and "src" in err[k], (k, err[k])
    for k in ("dst_rows_over", "src_rows_over", "mask_rows_over", "rows_come_before_blits"):
        assert rc[k] == UNSUPPORTED and "rows" in err[k], (k, err[k])
    for k in ("blits_null", "blits_come_before_aliasing"):
        assert rc[k] == INVALID and "blits is NULL" in err[k], (k, err[k])
    assert rc["aliasing_comes_before_opacity"] == INVALID and "overlap in memory" in err["aliasing_comes_before_opacity"]
    assert rc["opacity_256"] == INVALID and rc["invert_2"] == INVALID and rc["invert_2_on_an_empty_blit"] == INVALID
    assert "opacity" in err["opacity_comes_before_invert"] and "invert" in err["invert_comes_before_leaving"]
    assert "leaves the layer" in err["layer_out_comes_before_mask_out"] and "leaves the layer" in err["leaving_comes_before_overlap"]
    for k in ("mask_one_element_out_right", "mask_one_row_out_below", "mask_out_when_erasing"):
        assert rc[k] == INVALID and "leaves the mask" in err[k], (k, err[k])
    assert rc["source_last_column_in"] == 0 and rc["source_one_pixel_out_right"] == INVALID and rc["source_one_pixel_out_below"] == INVALID
    assert rc["too_many_tiles"] == UNSUPPORTED and "tiles" in err["too_many_tiles"]
    assert rc["pitch_max"] == 0 and rc["tall_image_last_rows"] == 0 and rc["plane_odd_pointer_is_valid"] == 0
    # the overlap rule; the message names the first pair
    assert rc["two_overlap_by_one_pixel"] == INVALID and rc["overlap_with_an_opacity_0_blit"] == INVALID and rc["overlap_only_before_clipping"] == 0
    assert "blits 1 and 2" in err["overlap_names_the_first_pair"]
    # layer and mask may alias, the destination may alias neither
    assert rc["layer_and_mask_the_same_image"] == 0 and rc["layer_and_plane_overlap"] == 0
    assert "layer and the destination" in err["dst_is_the_layer"] and "layer and the destination" in err["layer_overlap_comes_before_mask_overlap"]
    for k in ("dst_is_the_mask", "dst_is_the_mask_when_erasing", "dst_in_the_masks_last_byte", "dst_in_the_planes_last_bytes"):
        assert rc[k] == INVALID and "mask and the destination" in err[k], (k, err[k])
    assert rc["dst_behind_the_mask"] == 0 and rc["dst_behind_the_plane"] == 0 and rc["plane_ends_at_dst"] == 0
    # clipping: negative and out-of-range offsets
    assert tiles["negative_offsets"][0][2:7] == (0, 92, 34, 5, 7) and tiles["negative_offsets"][0][8:] == (7, 10, 0)
    assert tiles["erase_ignores_src_xy_and_size"] == [(0, 0, 0, 27, 16, 3, 4, 255 | DST_VEC | MASK_VEC, 8, 10, 0)]
    assert len(tiles["partly_outside_right_bottom"]) == 2
    for k in ("wholly_outside_right", "wholly_outside_above", "wholly_outside_left_by_min", "far_right_max", "zero_width_anywhere", "no_blits", "all_opacity_0"):
        assert rc[k] == 0 and tiles[k] == [], k
    for w in (1, 3, 64, 257):
        assert len(tiles[f"width_{w}"]) == (2 if w == 257 else 1) and len(tiles[f"width_{w}_at_x3"]) == 2 * (2 if w == 257 else 1)
        assert all(t[0] % 4 == 0 and t[5] == t[0] - 2 and t[8] == t[0] - 1 for t in tiles[f"width_{w}_at_x3"])    # x0 = 3: layer column 1, mask column 2
    # the tile table of a multi-blit call: blit by blit, none for opacity 0 or an empty blit; opacity and invert per tile
    assert [(t[0], t[1], t[7] & 255, t[10]) for t in tiles["multi_blit"]] == [(8, 10, 255, 0), (28, 10, 128, 1), (8, 20, 1, 0), (60, 5, 254, 1), (60, 21, 254, 1), (60, 37, 254, 1)]
    assert len(tiles["opacity_0_has_no_tile"]) == 1
    # the three vector flags, pointers and pitches on and off their grids
    flags = {k: tiles[k][0][7] & ~255 for k in tiles if tiles[k]}
    assert flags["whole_layer_aligned"] == flags["whole_plane_aligned"] == DST_VEC | SRC_VEC | MASK_VEC
    assert flags["erase_plane_aligned"] == DST_VEC | MASK_VEC and flags["erase_layer_mask_srgb"] == DST_VEC | MASK_VEC
    assert flags["negative_offsets"] == 0 and flags["negative_offsets_aligned_rows"] == DST_VEC | MASK_VEC     # mask column 3 + 5
    assert flags["dst_4_aligned_only"] == SRC_VEC | MASK_VEC and flags["src_4_aligned_only"] == DST_VEC | MASK_VEC
    assert flags["mask_4_aligned_only"] == DST_VEC | SRC_VEC and flags["mask_rows_off_the_grid"] == DST_VEC | SRC_VEC
    assert flags["src_rows_off_the_grid"] == DST_VEC | MASK_VEC
    assert flags["src_x_unaligned"] == DST_VEC | MASK_VEC and flags["mask_x_unaligned"] == DST_VEC | SRC_VEC
    assert flags["all_match_dst_x_mod_4"] == DST_VEC | SRC_VEC | MASK_VEC
    for off in range(4):
        for pitch in range(320, 324):
            t = tiles[f"plane_at_{off}_pitch_{pitch}"]
            # the first blit's column is 0: on the grid with the pointer; the second's makes up for the pointer's offset
            assert [bool(x[7] & MASK_VEC) for x in t] == [pitch % 4 == 0 and off == 0, pitch % 4 == 0], (off, pitch)
    assert flags["plane_pointer_plus_column_on_the_grid"] == DST_VEC | SRC_VEC | MASK_VEC and flags["plane_odd_pointer_is_valid"] == 0


def test_the_blit_struct():
    """fr_layer_mask_blit as the ctypes structure and as the numpy row make_mask_blits builds; the two flags"""
    assert (fr.FR_MASK_PLANE, fr.FR_MASK_ERASE) == (4, 8)
    table = fr.make_mask_blits([(1, 2, 30, 40, -5, -6, 7, 8, 200, 1)])
    assert table.shape == (1,) and table.dtype.itemsize == C.sizeof(_lib.LayerMaskBlit) == 40
    raw = _lib.LayerMaskBlit.from_buffer_copy(table.tobytes())
    assert tuple(getattr(raw, n) for n, _ in _lib.LayerMaskBlit._fields_) == (1, 2, 30, 40, -5, -6, 7, 8, 200, 1)
    assert np.dtype(_lib.LayerMaskBlit).names == ("src_x", "src_y", "w", "h", "dst_x", "dst_y", "mask_x", "mask_y", "opacity", "invert")

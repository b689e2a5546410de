"""The host side of fr_layer_lcd (csrc/fr_layer_lcd_plan.cpp) on the CPU: host/layer_lcd_selftest prints, for each case, the
inputs and what the builder made of them: the filter, the clipped rectangles and the tile table, or the refusal.  Every line
is compared with a restatement of the checks in the header's order, the clipping, the overlap rule and the tiling written
here from include/fr_raster.h and the comments of fr_layer_lcd_plan.hpp, computed from the inputs the line itself names; the
program checks the properties the kernel relies on by itself and fails if one does not hold."""
import host_selftest
import layer_ref as lr

TILE_W, TILE_H, LANE_PX, DST_VEC, SRC_VEC = 256, 16, 4, 0x100, 0x200
INVALID, UNSUPPORTED = -1, -4


def _lines():
    return host_selftest.cases("layer_lcd_selftest")


def _rows(text):
    return [] if text == "-" else [tuple(int(v) for v in r.split(",")) for r in text.split(";")]


def _expect(inp, null_blits):
    """the restatement: (rc, a word of the message) or (0, (w, clips, tiles))"""
    cov, dst, cs, cr, ds, dr, flags = (int(v) for v in inp["in"].split(","))
    blits = _rows(inp["blits"])
    W = (8, 77, 86, 77, 8) if inp["weights"] == "default" else tuple(int(v) for v in inp["weights"].split(","))
    if flags & ~3:
        return INVALID, "flag"
    if cov == 0:
        return INVALID, "cov is NULL"
    if cs > 1 << 26:
        return INVALID, "cov: row pitch"
    if dst == 0 or dst % 4 or ds > 1 << 26:
        return INVALID, "dst"
    if cr >= 1 << 31 or dr >= 1 << 31:
        return UNSUPPORTED, "rows"
    if blits and null_blits:
        return INVALID, "blits is NULL"
    if sum(W) != 256:
        return INVALID, "weights"
    clips = []
    for sx, sy, w, h, dx, dy, *_ in blits:
        if w and h and (sx + 3 * w > cs or sy + h > cr):
            return INVALID, "leaves the plane"
        clips.append(lr.clip((0, sy, w, h, dx, dy, 255), ds, dr))
    for i, a in enumerate(clips):
        for b in clips[i + 1:]:
            if a and b and a[0] < b[2] and b[0] < a[2] and a[1] < b[3] and b[1] < a[3]:
                return INVALID, "overlap in the destination"
    if cov < dst + 4 * ds * dr and dst < cov + cs * cr:
        return INVALID, "overlap in memory"
    n = 0
    for c in clips:
        if c:
            tx0 = c[0] - c[0] % LANE_PX
            n += -(-(c[2] - tx0) // TILE_W) * -(-(c[3] - c[1]) // TILE_H)
    if n > 1 << 22:
        return UNSUPPORTED, "tiles"
    tiles = []
    for c, b in zip(clips, blits):
        if c is None:
            continue
        x0, y0, x1, y1, u0, sy = c
        sx, w = b[0], b[2]
        rgba = b[6] | b[7] << 8 | b[8] << 16 | b[9] << 24
        tx0 = x0 - x0 % LANE_PX
        sq0 = sx + 3 * (u0 - (x0 - tx0))
        vec = (DST_VEC if dst % 16 == 0 and ds % 4 == 0 else 0) | (SRC_VEC if cs % 4 == 0 and (cov + sq0) % 4 == 0 else 0)
        for y in range(y0, y1, TILE_H):
            for x in range(tx0, x1, TILE_W):
                tiles.append((x, y, x0, x1, y1, sy + y - y0, sq0 + 3 * (x - tx0), sx, sx + 3 * w, rgba, vec))
    return 0, (W, [c or (0, 0, 0, 0, 0, 0) for c in clips], tiles)


def test_every_line_matches_the_restatement():
    lines = _lines()
    assert len(lines) >= 75
    for name, (inp, null_blits, tail) in lines.items():
        rc, want = _expect(inp, null_blits)
        assert int(inp["rc"]) == rc, (name, inp["rc"], rc, tail)
        if rc:
            assert tail.startswith("err=") and want in tail, (name, tail, want)      # the rule that refused it: the order
            continue
        got = dict(f.split("=", 1) for f in tail.split(" "))
        assert (tuple(int(v) for v in got["w"].split(",")), _rows(got["clips"]), _rows(got["tiles"])) == want, name


def test_every_refusal_of_the_header_has_a_case_in_order():
    L = _lines()
    rc = {k: int(v[0]["rc"]) for k, v in L.items()}
    refused = [k for k in L if rc[k]]
    for k, code in (("unknown_flag_4", INVALID), ("text_flag_bits", INVALID), ("cov_null", INVALID), ("cov_pitch_over", INVALID), ("dst_null", INVALID),
                    ("dst_not_4_aligned", INVALID), ("dst_pitch_over", INVALID), ("dst_rows_over", UNSUPPORTED), ("cov_rows_over", UNSUPPORTED),
                    ("blits_null", INVALID), ("weights_sum_255", INVALID), ("weights_sum_257", INVALID), ("weights_sum_wraps_uint16", INVALID),
                    ("weights_refused_without_blits", INVALID), ("window_one_element_out_right", INVALID), ("window_one_row_out_below", INVALID),
                    ("window_wraps_uint32", INVALID), ("window_width_wraps_uint32", INVALID), ("two_overlap_by_one_pixel", INVALID),
                    ("aliasing_same_memory", INVALID), ("aliasing_last_byte", INVALID), ("aliasing_image_first", INVALID), ("tiles_over", UNSUPPORTED),
                    ("tiles_over_by_the_lead", UNSUPPORTED)):
        assert rc[k] == code, k
    order = [k for k in refused if k.startswith("order_")]
    assert len(order) == 9
    # FR_LCD_BGR is a known bit here
    assert rc["srgb_and_bgr"] == 0


def test_the_named_cases():
    L = _lines()
    rc = {k: int(v[0]["rc"]) for k, v in L.items()}
    tiles = {k: _rows(dict(f.split("=", 1) for f in v[2].split(" "))["tiles"]) for k, v in L.items() if rc[k] == 0}
    for k in ("wholly_outside_right", "wholly_outside_above", "wholly_outside_left_by_min", "far_right_max", "zero_width_anywhere", "no_blits", "no_blits_null",
              "overlap_only_before_clipping"):
        assert tiles[k] == [], k
    # negative offsets: the window's pixel 5 lands on column 0, its elements start at 15; rows from plane row 7
    assert tiles["negative_offsets"][0][:9] == (0, 0, 0, 92, 34, 7, 15, 0, 291)
    # a rectangle at x = 3 from element 1: the tile starts three pixels, nine elements, to the left
    assert all(t[0] % 4 == 0 for ts in tiles.values() for t in ts)
    assert [t[6] for t in tiles["width_257_at_x3"][:2]] == [-8, 760] and len(tiles["width_257_at_x3"]) == 4
    assert len(tiles["width_257"]) == 2 and len(tiles["width_64"]) == 1
    # dwords only where cov + src_x (here the lead is 0) and the pitch are multiples of 4
    for sx in range(4):
        for pitch in (900, 901, 902, 903):
            assert bool(tiles[f"src_x_{sx}_pitch_{pitch}"][0][10] & SRC_VEC) == (sx == 0 and pitch == 900), (sx, pitch)
    for off in (1, 2, 3):
        assert tiles[f"cov_off_{off}"][0][10] & SRC_VEC
    assert tiles["whole_plane_aligned"][0][10] == DST_VEC | SRC_VEC and tiles["dst_4_aligned_only"][0][10] == SRC_VEC
    assert tiles["negative_offsets"][0][10] == 0 and tiles["negative_offsets_aligned_rows"][0][10] == DST_VEC
    # the colour travels with every tile of its blit
    assert [t[9] for t in tiles["two_touching"]] == [0xffffffff, 0x04030201, 0xffffffff]
    assert tiles["window_last_element_in"][0][6:9] == (609, 609, 900)
    assert rc["adjacent_images"] == 0 and rc["pitch_max"] == 0 and rc["tall_image_last_rows"] == 0


def test_blit_struct_layout():
    """fr_lcd_blit as the ctypes structure and as the numpy row make_lcd_blits builds"""
    import ctypes as C

    import font_renderer_amd as fr
    from font_renderer_amd import _lib
    table = fr.make_lcd_blits([(1, 2, 30, 40, -5, -6, (9, 8, 7, 250))])
    assert table.shape == (1,) and table.dtype.itemsize == C.sizeof(_lib.LcdBlit) == 28
    raw = _lib.LcdBlit.from_buffer_copy(table.tobytes())
    assert (raw.src_x, raw.src_y, raw.w, raw.h, raw.dst_x, raw.dst_y, tuple(raw.rgba)) == (1, 2, 30, 40, -5, -6, (9, 8, 7, 250))
    assert (fr.FR_LCD_BGR, fr.FR_LCD_TAPS, fr.FR_LAYER_SRGB) == (2, 5, 1)

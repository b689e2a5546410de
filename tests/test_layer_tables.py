"""The host side of fr_layer_over (csrc/fr_layer_plan.cpp) on the CPU: host/layer_selftest prints, for each case, the inputs
and what the builder made of them: the clipped rectangles and the tile table, or the refusal.  Every line is compared with
a restatement of the clipping, the overlap rule and the tiling written here from include/fr_raster.h and the comments of
fr_layer_plan.hpp, computed from the inputs the line itself names; the program checks the coverage properties of its
tables on its own and fails if one does not hold."""
import pytest

import host_selftest
import layer_ref as lr

TILE_W, TILE_H, LANE_PX, DST_VEC, SRC_VEC = 256, 16, 4, 0x100, 0x200


def _lines():
    return host_selftest.cases("layer_selftest")


def _rows(text):
    return [] if text == "-" else [tuple(int(v) for v in r.split(",")) for r in text.split(";")]


def _expect(inp, null_blits):
    """the restatement: (rc, None) or (0, (opacity, pixels, clips, tiles))"""
    src, dst, ss, sr, ds, dr, flags = (int(v) for v in inp["in"].split(","))
    blits = _rows(inp["blits"])
    if flags & ~1:
        return -1, None
    for p, stride in ((src, ss), (dst, ds)):
        if p == 0 or p % 4 or stride > 1 << 26:
            return -1, None
    if sr >= 1 << 31 or dr >= 1 << 31:
        return -4, None
    if blits and null_blits:
        return -1, None
    if src < dst + 4 * ds * dr and dst < src + 4 * ss * sr:
        return -1, None
    clips = []
    for sx, sy, w, h, dx, dy, o in blits:
        if o > 255:
            return -1, None
        if w and h and (sx + w > ss or sy + h > sr):
            return -1, None
        clips.append(lr.clip((sx, sy, w, h, dx, dy, o), ds, dr))
    for i, a in enumerate(clips):
        for b in clips[i + 1:]:
            if a and b and a[0] < b[2] and b[0] < a[2] and a[1] < b[3] and b[1] < a[3]:
                return -1, None
    dvec = dst % 16 == 0 and ds % 4 == 0
    svec = src % 16 == 0 and ss % 4 == 0
    tiles, pixels, opacity = [], 0, 0
    for c, b in zip(clips, blits):
        if c is None:
            continue
        x0, y0, x1, y1, sx, sy = c
        pixels += (x1 - x0) * (y1 - y0)
        o = b[6]
        if o == 0:
            continue
        opacity |= o != 255
        tx0 = x0 - x0 % LANE_PX
        ov = o | (DST_VEC if dvec else 0) | (SRC_VEC if svec and (sx - (x0 - tx0)) % LANE_PX == 0 else 0)
        for y in range(y0, y1, TILE_H):
            for x in range(tx0, x1, TILE_W):
                tiles.append((x, y, x0, x1, y1, sx - (x0 - x), sy + y - y0, ov))
    return 0, (int(opacity), pixels, [c or (0, 0, 0, 0, 0, 0) for c in clips], tiles)


def test_every_line_matches_the_restatement():
    lines = {k: v for k, v in _lines().items() if not k.startswith("window/")}
    assert len(lines) >= 45
    for name, (inp, null_blits, tail) in lines.items():
        rc, want = _expect(inp, null_blits)
        assert int(inp["rc"]) == rc, (name, inp["rc"], rc, tail)
        if rc:
            assert tail.startswith("err=") and len(tail) > 4, (name, tail)
            continue
        got = dict(f.split("=", 1) for f in tail.split(" "))
        assert (int(got["opacity"]), int(got["pixels"]), _rows(got["clips"]), _rows(got["tiles"])) == want, name


def test_the_named_cases():
    L = _lines()
    rc = {k: int(v[0]["rc"]) for k, v in L.items()}
    tiles = {k: _rows(dict(f.split("=", 1) for f in v[2].split(" "))["tiles"]) for k, v in L.items() if rc[k] == 0 and not k.startswith("window/")}
    # negative offsets, partly and wholly outside
    assert rc["negative_offsets"] == 0 and tiles["negative_offsets"][0][2:7] == (0, 92, 34, 5, 7)
    assert rc["partly_outside_right_bottom"] == 0 and len(tiles["partly_outside_right_bottom"]) == 2
    for k in ("wholly_outside_right", "wholly_outside_above", "wholly_outside_left_by_min", "far_right_max", "zero_width_anywhere", "no_blits"):
        assert rc[k] == 0 and tiles[k] == [], k
    # the widths: one tile column up to 256 pixels from the aligned origin, two beyond
    for w in (1, 3, 63, 64, 65, 257):
        assert rc[f"width_{w}"] == 0 and len(tiles[f"width_{w}"]) == (2 if w == 257 else 1)
        assert rc[f"width_{w}_at_x3"] == 0 and len(tiles[f"width_{w}_at_x3"]) == 2 * (2 if w == 257 else 1)
        assert all(t[0] % 4 == 0 and t[5] == t[0] - 2 for t in tiles[f"width_{w}_at_x3"])       # x0 = 3 from layer column 1
    # touching is valid, one shared pixel is not, also under an opacity of 0; what clipping removes cannot overlap
    assert rc["two_touching"] == 0 and rc["overlap_only_before_clipping"] == 0
    assert rc["two_overlap_by_one_pixel"] == -1 and rc["overlap_with_an_opacity_0_blit"] == -1
    # the layer's edge, the opacity, aliasing, alignment, flags, the pitch
    assert rc["source_last_column_in"] == 0 and rc["source_one_pixel_out_right"] == -1 and rc["source_one_pixel_out_below"] == -1
    assert rc["opacity_256"] == -1 and rc["aliasing_same_image"] == -1 and rc["aliasing_last_byte"] == -1 and rc["adjacent_images"] == 0
    assert rc["src_not_4_aligned"] == -1 and rc["dst_not_4_aligned"] == -1 and rc["src_null"] == -1 and rc["dst_null"] == -1
    assert rc["blits_null"] == -1 and rc["unknown_flag_2"] == -1 and rc["text_flag_bits"] == -1
    assert rc["pitch_max"] == 0 and rc["pitch_over"] == -1 and rc["rows_over"] == -4
    # the 16-byte flags: only with 16-byte aligned rows, and for the layer only where its column matches modulo 4
    assert tiles["whole_layer_aligned"][0][7] == 255 | DST_VEC | SRC_VEC
    assert tiles["negative_offsets"][0][7] == 255 and tiles["negative_offsets_aligned_rows"][0][7] == 255 | DST_VEC
    assert tiles["dst_4_aligned_only"][0][7] == 255 | SRC_VEC and tiles["src_4_aligned_only"][0][7] == 255 | DST_VEC
    assert tiles["src_x_unaligned"][0][7] == 255 | DST_VEC and tiles["src_x_matches_dst_x_mod_4"][0][7] == 255 | DST_VEC | SRC_VEC
    assert [t[7] & 255 for t in tiles["opacity_255_and_128"]] == [255, 128] and len(tiles["opacity_0_has_no_tile"]) == 1


@pytest.mark.parametrize("name,rc", [("window/inside", 0), ("window/whole_row", 0), ("window/wider_than_rows", -1), ("window/null", -1),
                                     ("window/not_4_aligned", -1), ("window/empty", 0), ("window/pitch_over", -1),
                                     ("window/too_many_tiles", -4)])
def test_unpremultiply_window(name, rc):
    inp, _, tail = _lines()[name]
    assert int(inp["rc"]) == rc and (tail == "ok" if rc == 0 else tail.startswith("err=")), (name, tail)

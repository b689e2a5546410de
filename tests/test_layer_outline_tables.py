"""The host side of fr_layer_outline (csrc/fr_layer_outline_plan.cpp) on the CPU: host/layer_outline_selftest prints, for each
case, the inputs and what the planner made of them: the rectangle in window coordinates, its cut to the reach, the stores'
lead and the tile counts, or the refusal; and for a list of radii the weight table.  Every line is compared with a
restatement of the checks, the rectangles and the weights written here from include/fr_raster.h, computed from the inputs
the line itself names; the program checks on its own that the packed table decodes to the weights and fails if not."""
import host_selftest
import layer_outline_ref as orf

TILE = 64


def _lines():
    plans, tables = {}, {}
    for name, rest in host_selftest.named("layer_outline_selftest").items():
        if name.startswith("table/"):
            tables[int(name[6:])] = dict(f.split("=", 1) for f in rest.split(" "))
        else:
            head, tail = rest.split(" | ", 1)
            plans[name] = (dict(f.split("=", 1) for f in head.split(" ")), tail)
    return plans, tables


def _cut(a, b):
    r = (max(a[0], b[0]), max(a[1], b[1]), min(a[2], b[2]), min(a[3], b[3]))
    return None if r[0] >= r[2] or r[1] >= r[3] else r


def _expect(inp):
    """the restatement, in the header's order: (rc, None) or (0, (nothing, zeros, want, live, vec, lead, tiles, reach))"""
    src, dst, ss, sr, ds, dr, flags = (int(v) for v in inp["in"].split(","))
    if flags & ~1:
        return -1, None
    for p, stride in ((src, ss), (dst, ds)):
        if p == 0 or p % 4 or stride > 1 << 26:
            return -1, None
    if sr >= 1 << 31 or dr >= 1 << 31:
        return -4, None
    if inp["outline"] == "null":
        return -1, None
    sx, sy, w, h, x, y, dw, dh, dx, dy, rho, kind = (int(v) for v in inp["outline"].split(","))
    if w and h and (sx + w > ss or sy + h > sr):
        return -1, None
    if dw and dh and (x + dw > ds or y + dh > dr):
        return -1, None
    if rho > 256 or kind > 3:
        return -1, None
    if src < dst + 4 * ds * dr and dst < src + 4 * ss * sr:
        return -1, None
    if dw and dh and -(-(dw + 3) // TILE) * -(-dh // TILE) > 1 << 22:
        return -4, None
    want = (-dx, -dy, -dx + dw, -dy + dh)
    none = (0, 0, 0, 0)
    if not (dw and dh):
        return 0, (1, 0, want, none, 0, 0, (0, 0), 0)
    vec = int(ds % 4 == 0)
    lead = (dst // 4 + y * ds + x) % 4 if vec else 0
    tiles = (-(-(dw + lead) // TILE), -(-dh // TILE))
    R = orf.reach(rho)
    live = None
    if w and h:
        live = _cut(want, (-R, -R, w + R, h + R) if kind in (orf.GROW, orf.RING) else (0, 0, w, h))
    if live is None or (rho == 0 and kind in (orf.RING, orf.INNER)):
        return 0, (0, 1, want, none, vec, lead, tiles, 0)
    return 0, (0, 0, want, live, vec, lead, tiles, R)


def test_every_line_matches_the_restatement():
    plans, _ = _lines()
    assert len(plans) >= 90
    for name, (inp, tail) in plans.items():
        rc, want = _expect(inp)
        assert int(inp["rc"]) == rc, (name, inp["rc"], rc, tail)
        if rc:
            assert tail.startswith("err=") and len(tail) > 4, (name, tail)
            continue
        got = dict(f.split("=", 1) for f in tail.split(" "))
        ints = lambda key: tuple(int(v) for v in got[key].split(","))
        assert (int(got["nothing"]), int(got["zeros"]), ints("want"), ints("live"), int(got["vec"]), int(got["lead"]), ints("tiles"),
                int(got["reach"])) == want, name


def test_the_tables():
    """the weights are the header's K; a row's core, rim and running-maximum level follow from them"""
    _, tables = _lines()
    assert {0, 1, 15, 16, 17, 256} <= set(tables)
    for rho, t in tables.items():
        R = orf.reach(rho)
        R4 = (R + 3) // 4 * 4
        n = 2 * R + 1
        assert (int(t["reach"]), int(t["reach4"]), int(t["words"])) == (R, R4, R4 // 2 + 1)
        levels = 0
        K = [[orf.weight(rho, i, j) for i in range(-R, R + 1)] for j in range(-R, R + 1)]
        assert bytes.fromhex(t["k"]) == bytes(v for row in K for v in row), rho
        rows = [tuple(int(v) for v in r.split(",")) for r in t["rows"].split(";")]
        assert len(rows) == n
        for row, k in zip(rows, K):
            right = k[R:]                                       # K(0, j), K(1, j), ..: it does not increase
            core = max((i for i, v in enumerate(right) if v == 255), default=-1)
            rim = sum(1 for v in right if 0 < v < 255)
            level = (2 * core + 1).bit_length() - 1 if core >= 0 else 0        # floor(log2(2 core + 1))
            levels = max(levels, level)
            assert row == (core, rim, level), (rho, row)
            assert all(v == 0 for v in right[core + rim + 1:]) and rim <= 7
        assert int(t["levels"]) == levels and (levels == 5) == (rho == 256)


def test_the_named_cases():
    """every refusal of the header at its limit and one past it, in the header's order, and the cases the launch depends on"""
    L, _ = _lines()
    rc = {k: int(v[0]["rc"]) for k, v in L.items()}
    out = {k: dict(f.split("=", 1) for f in v[1].split(" ")) for k, v in L.items() if rc[k] == 0}
    assert rc["typical"] == 0 and rc["typical_srgb"] == 0 and out["typical"]["reach"] == "3" and out["typical"]["live"] == "0,0,100,44"
    # the radius and the kind, after the window and the rectangle, before the aliasing
    assert rc["radius_256"] == 0 and out["radius_256"]["reach"] == "16"
    assert rc["radius_257"] == rc["kind_4"] == rc["radius_before_kind"] == rc["zero_rect_bad_radius"] == -1
    assert "radius" in L["radius_257"][1] and "kind" in L["kind_4"][1] and "radius" in L["radius_before_kind"][1]
    assert "window" in L["window_before_radius"][1] and "radius" in L["radius_before_aliasing"][1]
    assert out["radius_1"]["reach"] == out["radius_16"]["reach"] == "1" and out["radius_17"]["reach"] == "2"
    # reach: R = 3 around the 97 x 41 window for GROW and RING, the window itself for INNER and SHRINK
    for kind in (0, 1):
        assert out["just_in_reach_kind%d" % kind]["zeros"] == "0" and out["just_out_of_reach_kind%d" % kind]["zeros"] == "1"
        assert out["in_reach_above_kind%d" % kind]["zeros"] == "0" and out["out_of_reach_above_kind%d" % kind]["zeros"] == "1"
        assert out["padded_by_reach_kind%d" % kind]["live"] == "-3,-3,100,44"
    for kind in (2, 3):
        assert out["last_window_column_kind%d" % kind]["zeros"] == "0" and out["first_column_beyond_kind%d" % kind]["zeros"] == "1"
        assert out["just_in_reach_kind%d" % kind]["zeros"] == "1" and out["in_reach_above_kind%d" % kind]["zeros"] == "1"
        assert out["padded_by_reach_kind%d" % kind]["live"] == "0,0,97,41"
    assert [out["radius_0_kind%d" % k]["zeros"] for k in range(4)] == ["0", "1", "1", "0"]
    assert out["inner_cut_to_the_window"]["live"] == "0,0,97,41" and out["inner_cut_to_the_window"]["tiles"] == "3,2"
    assert out["offset_int32_min"]["zeros"] == "1" and out["offset_int32_max"]["zeros"] == "1"
    # zero sizes
    assert all(out["zero_window_width_kind%d" % k]["zeros"] == "1" for k in range(4)) and out["zero_window_height"]["zeros"] == "1"
    assert out["zero_rect_width"]["nothing"] == "1" and out["zero_rect_height"]["nothing"] == "1"
    # the window and the rectangle against their images
    assert rc["window_last_column_in"] == 0 and rc["window_one_pixel_out_right"] == -1 and rc["window_one_pixel_out_below"] == -1
    assert rc["rect_last_column_and_row_in"] == 0 and rc["rect_one_pixel_out_right"] == -1 and rc["rect_one_pixel_out_below"] == -1
    assert rc["rect_x_wraps_32_bits"] == -1
    # the stores
    assert (out["lead_0"]["lead"], out["lead_1"]["lead"], out["lead_3_adds_a_tile_column"]["lead"], out["lead_from_the_pointer"]["lead"]) == ("0", "1", "3", "3")
    assert out["lead_1"]["tiles"] == "1,1" and out["lead_3_adds_a_tile_column"]["tiles"] == "2,1"
    assert out["rows_of_131"]["vec"] == "0" and out["rows_of_131"]["lead"] == "0" and out["rows_of_131"]["tiles"] == "1,1"
    # pointers, flags, aliasing, pitches, rows, tiles
    assert rc["src_null"] == rc["dst_null"] == rc["outline_null"] == rc["src_not_4_aligned"] == rc["dst_not_4_aligned"] == -1
    assert "src" in L["src_null"][1] and "dst" in L["dst_null"][1] and "outline" in L["outline_null"][1]
    assert rc["unknown_flag_2"] == rc["text_flag_bits"] == -1 and rc["flag_before_null"] == -1 and "flag" in L["flag_before_null"][1]
    assert rc["aliasing_same_image"] == rc["aliasing_last_byte"] == -1 and rc["adjacent_images"] == 0
    assert rc["src_pitch_max"] == 0 and rc["src_pitch_over"] == -1 and rc["dst_pitch_max"] == 0 and rc["dst_pitch_over"] == -1
    assert rc["src_rows_max"] == 0 and rc["src_rows_over"] == -4 and rc["dst_rows_max"] == 0 and rc["dst_rows_over"] == -4
    assert rc["rect_tiles_at_2_22"] == 0 and out["rect_tiles_at_2_22"]["tiles"] == "2048,2048"
    assert rc["rect_tiles_over_by_a_column"] == rc["rect_tiles_over_by_a_row"] == rc["rect_tiles_over_out_of_reach"] == -4
    assert "tiles" in L["rect_tiles_over_by_a_row"][1]

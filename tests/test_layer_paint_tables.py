"""The host side of fr_layer_paint (csrc/fr_layer_paint_plan.cpp) on the CPU: host/layer_paint_selftest prints, for each
case, the inputs and what the builder made of them: the clipped rectangle, the tiles, the coefficients and the colour
table, or the refusal.  Every line is compared with a restatement of the checks and the clipping written here from
include/fr_raster.h, with the coefficients and the table of the twin (tests/layer_paint_ref.py, itself held to exact
fractions by tests/test_layer_paint_ref.py), computed from the inputs the line itself names; the program checks the
properties of its plan on its own and fails if one does not hold."""
import host_selftest
import layer_paint_ref as pr

TILE_W, TILE_H, MAX_TILES = 256, 16, 1 << 22


def _lines():
    return host_selftest.cases("layer_paint_selftest")


def _ints(text):
    return [int(v) for v in text.split(",")]


def _stops(text):
    return [] if text == "-" else [(r[0], tuple(r[1:])) for r in map(_ints, text.split(";"))]


def _expect(inp):
    """the restatement, in the header's order: (rc, None), (0, "nothing") or (0, (clip, tiles, c, table))"""
    src, ss, sr, dst, ds, dr, flags = _ints(inp["in"])
    if flags & ~1:
        return -1, None
    if dst == 0 or dst % 4 or ds > 1 << 26:
        return -1, None
    if src and (src % 4 or ss > 1 << 26):
        return -1, None
    if not src and (ss or sr):
        return -1, None
    if sr >= 1 << 31 or dr >= 1 << 31:
        return -4, None
    if inp["paint"] == "null":
        return -1, None
    sx, sy, w, h, dx, dy, kind, spread, x0, y0, x1, y1, n = _ints(inp["paint"])
    stops = _stops(inp["stops"])
    if src and w and h and (sx + w > ss or sy + h > sr):
        return -1, None
    if not src and (sx or sy):
        return -1, None
    if kind > 1 or spread > 2 or not 1 <= n <= 8:
        return -1, None
    assert len(stops) == n
    if any(s[0] > 65536 for s in stops) or any(b[0] < a[0] for a, b in zip(stops, stops[1:])):
        return -1, None
    if kind == 0 and (x0, y0) == (x1, y1):
        return -1, None
    if kind == 1 and (x1 <= 0 or y1 != 0):
        return -1, None
    if src and src < dst + 4 * ds * dr and dst < src + 4 * ss * sr:
        return -1, None
    if any(abs(v) > 1 << 26 for v in (x0, y0, x1, y1)):
        return -4, None
    if kind == 0 and (x1 - x0) ** 2 + (y1 - y0) ** 2 < 4096 or kind == 1 and x1 < 64:
        return -4, None
    c = pr.clip((sx, sy, w, h), (dx, dy), ds, dr)
    if c is None:
        return 0, "nothing"
    X0, Y0, X1, Y1, csx, csy = c
    if kind == 1 and any(abs(64 * X + 32 - x0) >= 1 << 27 or abs(64 * Y + 32 - y0) >= 1 << 27 for X in (X0, X1 - 1) for Y in (Y0, Y1 - 1)):
        return -4, None
    tx0 = X0 // 4 * 4
    nx, ny = -(-(X1 - tx0) // TILE_W), -(-(Y1 - Y0) // TILE_H)
    if nx * ny > MAX_TILES:
        return -4, None
    sx0 = csx - (X0 - tx0)
    vec = (int(dst % 16 == 0 and ds % 4 == 0), int(bool(src) and src % 16 == 0 and ss % 4 == 0 and sx0 % 4 == 0))
    coeff = pr.linear_coefficients(x0, y0, x1, y1) if kind == 0 else (x0, y0, pr.radial_coefficient(x1))
    table = "".join("%02x%02x%02x%02x" % (a, b, g, r) for r, g, b, a in pr.table(stops).tolist())
    return 0, ([X0, Y0, X1, Y1, csx, csy], [tx0, nx, ny, sx0, *vec], list(coeff), table)


def _plan(tail):
    got = dict(f.split("=", 1) for f in tail.split(" "))
    return _ints(got["clip"]), _ints(got["tiles"]), _ints(got["c"]), got["table"]


def test_every_line_matches_the_restatement():
    lines = _lines()
    assert len(lines) >= 80
    drawn = 0
    for name, (inp, _, tail) in lines.items():
        rc, want = _expect(inp)
        assert int(inp["rc"]) == rc, (name, inp["rc"], rc, tail)
        if rc:
            assert tail.startswith("err=") and len(tail) > 4, (name, tail)
        elif want == "nothing":
            assert tail == "nothing", (name, tail)
        else:
            assert _plan(tail) == want, name
            drawn += 1
    assert drawn >= 25                                      # (the comparison above is not vacuous)


def test_the_named_cases():
    L = _lines()
    rc = {k: int(v[0]["rc"]) for k, v in L.items()}
    T = {k: _plan(v[2]) for k, v in L.items() if rc[k] == 0 and v[2] != "nothing"}
    for k in ("clipped_away_right", "clipped_away_above", "clipped_away_far", "zero_width", "zero_height_window_outside", "radial_too_far_but_clipped_away"):
        assert rc[k] == 0 and L[k][2] == "nothing", k
    assert T["linear_whole_image"][:2] == ([0, 0, 300, 40, 0, 0], [0, 2, 3, 0, 1, 1])          # two tiles across, three down
    assert T["margin"][:2] == ([5, 3, 295, 38, 3, 2], [4, 2, 3, 2, 1, 0]) and T["margin"][2] == [-(1 << 25), 1 << 25, 1 << 25]    # a dyadic 45 degrees
    assert T["negative_position"][0] == [0, 0, 293, 35, 7, 5] and T["over_the_right_and_bottom"][0] == [200, 30, 300, 40, 0, 0]
    assert T["rows301_no_vec"][1][4:] == [0, 1] and T["dst_4_aligned_only"][1][4:] == [0, 1] and T["src_4_aligned_only"][1][4:] == [1, 0]
    assert T["window_off_the_grid"][1][3:] == [1, 1, 0] and T["window_and_rectangle_off_alike"][1] == [8, 1, 3, 4, 1, 1] and T["no_layer"][1][5] == 0
    assert T["shortest_linear"][2] == [1 << 31, 1 << 32, 0] and T["shortest_radial"][2] == [0, 0, 1 << 54]
    assert T["radial_centre_at_the_limit"][0][:4] == [(1 << 20) - 300, 0, 1 << 20, 2] and T["far_pixels_linear"][1][:3] == [1 << 20, 2, 1]
    assert T["tiles_at_the_limit"][1][1] * T["tiles_at_the_limit"][1][2] == 1 << 22 and "linear_just_a_pixel" in T and "images_adjoin" in T
    assert T["one_stop"][3] == "c8070809" * 1024 and T["hard_edges_only"][3] == "ff0000ff" * 512 + "4dff0000" * 512
    # every refusal of the header, and the order of the checks: one case per rule, the earlier rule's code and message
    invalid = ("unknown_flag_2 text_flag_bits dst_null dst_not_4_aligned dst_pitch_over src_not_4_aligned src_pitch_over no_layer_with_stride no_layer_with_rows "
               "paint_null window_leaves_right window_leaves_below window_wraps_uint32 no_layer_with_src_x no_layer_with_src_y unknown_kind unknown_spread no_stops "
               "nine_stops offset_above_65536 offsets_decrease linear_length_0 radial_radius_0 radial_radius_negative radial_y1_set images_overlap refused_though_zero_size")
    unsupported = ("dst_rows_over src_rows_over geometry_x0_over geometry_y0_under geometry_radius_over geometry_y1_over linear_under_a_pixel radial_under_a_pixel "
                   "radial_corner_too_far radial_row_too_far tiles_over tiles_over_by_the_lead")
    assert all(rc[k] == -1 for k in invalid.split()) and all(rc[k] == -4 for k in unsupported.split())
    order = {"order_flag_before_dst": (-1, "flag"), "order_dst_before_src": (-1, "dst"), "order_src_before_rows": (-1, "src"), "order_rows_before_null_paint": (-4, "rows"),
             "order_window_before_kind": (-1, "window"), "order_kind_before_spread_before_stops": (-1, "kind"), "order_stops_before_length": (-1, "stops"),
             "order_length_before_overlap": (-1, "length"), "order_overlap_before_limits": (-1, "overlap"), "order_limits_before_short": (-4, "beyond"),
             "order_short_before_corner": (-4, "radius")}
    for k, (code, word) in order.items():
        assert rc[k] == code and word in L[k][2], (k, L[k][2])
    assert "centre" in L["radial_corner_too_far"][2] and "tiles" in L["tiles_over"][2]
    assert len(invalid.split()) + len(unsupported.split()) + len(order) == sum(1 for v in rc.values() if v)

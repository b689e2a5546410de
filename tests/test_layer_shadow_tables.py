"""The host side of fr_layer_shadow (csrc/fr_layer_shadow_plan.cpp) on the CPU: host/layer_shadow_selftest prints, for each
case, the inputs and what the planner made of them: the stage list with every stage's rectangle, the planes' sizes and the
reciprocal of the box division, or the refusal.  Every line is compared with a restatement of the checks and the rectangles
written here from include/fr_raster.h, computed from the inputs the line itself names; the program checks on its own that
every stage's rectangle lies inside its input's rectangle grown by the radius and fails if not."""
import host_selftest

TILE = 64


def _lines():
    out = {}
    for name, rest in host_selftest.named("layer_shadow_selftest").items():
        if not name.startswith("recip/"):
            head, tail = rest.split(" | ", 1)
            out[name] = (dict(f.split("=", 1) for f in head.split(" ")), tail)
    return out


def _cut(a, b):
    r = (max(a[0], b[0]), max(a[1], b[1]), min(a[2], b[2]), min(a[3], b[3]))
    return None if r[0] >= r[2] or r[1] >= r[3] else r


def _grow(a, k):
    return (a[0] - k, a[1] - k, a[2] + k, a[3] + k)


def _recip(r):
    W = (2 * r + 1) ** 2
    shift = W.bit_length() - 1
    return -(-(1 << (32 + shift)) // W), shift


def _expect(inp):
    """the restatement, in the header's order: (rc, None) or (0, (nothing, zeros, want, planes, stages))"""
    src, dst, ss, sr, ds, dr, flags = (int(v) for v in inp["in"].split(","))
    if flags & ~1:
        return -1, None
    for p, stride in ((src, ss), (dst, ds)):
        if p == 0 or p % 4 or stride > 1 << 26:
            return -1, None
    if sr >= 1 << 31 or dr >= 1 << 31:
        return -4, None
    if inp["shadow"] == "null":
        return -1, None
    sx, sy, w, h, x, y, dw, dh, dx, dy, s, r, p = (int(v) for v in inp["shadow"].split(","))
    if w and h and (sx + w > ss or sy + h > sr):
        return -1, None
    if dw and dh and (x + dw > ds or y + dh > dr):
        return -1, None
    if s > 8 or r > 32 or p > 3:
        return -1, None
    if src < dst + 4 * ds * dr and dst < src + 4 * ss * sr:
        return -1, None
    if dw and dh and -(-(dw + 3) // TILE) * -(-dh // TILE) > 1 << 22:
        return -4, None
    want = (-dx, -dy, -dx + dw, -dy + dh)
    if not (dw and dh):
        return 0, (1, 0, want, [0, 0], [])
    radii = ([s] if s else []) + ([r] * p if r else [])
    R = sum(radii)
    win = (0, 0, w, h)
    if not (w and h) or _cut(want, _grow(win, R)) is None:
        return 0, (0, 1, want, [0, 0], [])
    stages, planes, before = [], [0, 0], 0
    for k, rad in enumerate(radii):
        before += rad
        out = _cut(_grow(want, R - before), _grow(win, before))
        kind = 1 if k == 0 and s else 0
        pitch = 0
        if k + 1 < len(radii):
            pitch = -(-(out[2] - out[0]) // TILE) * TILE
            planes[k & 1] = max(planes[k & 1], pitch * (out[3] - out[1]))
        stages.append((kind, rad) + out + (pitch,) + (_recip(rad) if kind == 0 else (0, 0)))
    if sum(planes) > 1 << 30:
        return -4, None
    return 0, (0, 0, want, planes, stages)


def test_every_line_matches_the_restatement():
    lines = _lines()
    assert len(lines) >= 55
    for name, (inp, tail) in lines.items():
        rc, want = _expect(inp)
        assert int(inp["rc"]) == rc, (name, inp["rc"], rc, tail)
        if rc:
            assert tail.startswith("err=") and len(tail) > 4, (name, tail)
            continue
        got = dict(f.split("=", 1) for f in tail.split(" "))
        stages = [] if got["stages"] == "-" else [tuple(int(v) for v in st.split(",")) for st in got["stages"].split(";")]
        assert (int(got["nothing"]), int(got["zeros"]), tuple(int(v) for v in got["want"].split(",")), [int(v) for v in got["planes"].split(",")],
                stages) == want, name


def test_the_named_cases():
    """every refusal of the header at its limit and one past it, and the cases the kernels' launches depend on"""
    L = _lines()
    rc = {k: int(v[0]["rc"]) for k, v in L.items()}
    out = {k: dict(f.split("=", 1) for f in v[1].split(" ")) for k, v in L.items() if rc[k] == 0}
    n_stages = {k: 0 if v["stages"] == "-" else v["stages"].count(";") + 1 for k, v in out.items()}
    assert rc["typical"] == 0 and n_stages["typical"] == 4 and rc["typical_srgb"] == 0
    assert n_stages["no_stage"] == 0 and n_stages["radius_without_passes"] == 0 and n_stages["passes_without_radius"] == 0
    assert out["no_stage"]["zeros"] == "0" and n_stages["spread_only"] == 1 and n_stages["one_box"] == 1
    # the ranges of s, r and p
    assert rc["limits_8_32_3"] == 0 and n_stages["limits_8_32_3"] == 4
    assert rc["spread_9"] == rc["radius_33"] == rc["passes_4"] == rc["radius_33_without_passes"] == -1
    for k, word in (("spread_9", "spread"), ("radius_33", "blur_radius"), ("passes_4", "blur_passes")):
        assert word in L[k][1]
    # reach: R = 1 + 3 * 3 = 10 around the 97 x 41 window
    assert out["just_in_reach"]["zeros"] == "0" and out["just_out_of_reach"]["zeros"] == "1"
    assert out["in_reach_above"]["zeros"] == "0" and out["out_of_reach_above"]["zeros"] == "1"
    assert out["offset_int32_min"]["zeros"] == "1" and out["offset_int32_max"]["zeros"] == "1"
    # zero sizes
    assert out["zero_window_width"]["zeros"] == "1" and out["zero_window_height"]["zeros"] == "1"
    assert out["zero_rect_width"]["nothing"] == "1" and out["zero_rect_height"]["nothing"] == "1"
    # the window and the rectangle against their images
    assert rc["window_last_column_in"] == 0 and rc["window_one_pixel_out_right"] == -1 and rc["window_one_pixel_out_below"] == -1
    assert rc["rect_last_column_and_row_in"] == 0 and rc["rect_one_pixel_out_right"] == -1 and rc["rect_one_pixel_out_below"] == -1
    assert rc["rect_x_wraps_32_bits"] == -1
    # pointers, flags, aliasing, pitches, rows, planes
    assert rc["src_null"] == rc["dst_null"] == rc["shadow_null"] == rc["src_not_4_aligned"] == rc["dst_not_4_aligned"] == -1
    assert "src" in L["src_null"][1] and "dst" in L["dst_null"][1] and "shadow" in L["shadow_null"][1]
    assert rc["both_4_aligned_only"] == 0
    assert rc["unknown_flag_2"] == rc["text_flag_bits"] == -1 and rc["flag_before_null"] == -1 and "flag" in L["flag_before_null"][1]
    assert rc["aliasing_same_image"] == rc["aliasing_last_byte"] == -1 and rc["adjacent_images"] == 0
    assert rc["src_pitch_max"] == 0 and rc["src_pitch_over"] == -1 and rc["dst_pitch_max"] == 0 and rc["dst_pitch_over"] == -1
    assert rc["src_rows_max"] == 0 and rc["src_rows_over"] == -4 and rc["dst_rows_max"] == 0 and rc["dst_rows_over"] == -4
    assert rc["planes_at_2_30"] == 0 and sum(int(v) for v in out["planes_at_2_30"]["planes"].split(",")) == 1 << 30
    assert rc["planes_over_2_30"] == -4
    assert rc["rect_tiles_at_2_22"] == 0 and n_stages["rect_tiles_at_2_22"] == 1
    assert rc["rect_tiles_over_by_a_column"] == rc["rect_tiles_over_by_a_row"] == rc["rect_tiles_over_out_of_reach"] == -4
    assert "tiles" in L["rect_tiles_over_by_a_row"][1]

// layer_paint_selftest.cpp — the host side of fr_layer_paint (csrc/fr_layer_paint_plan.cpp) on the CPU: links
// fr_layer_paint_plan.o and nothing else of the library.  No GPU; the device pointers are made-up integers.  It prints one
// line per case,
//   <case> rc=<code> in=<src>,<src stride>,<src rows>,<dst>,<dst stride>,<dst rows>,<flags>
//          paint=<src_x>,<src_y>,<w>,<h>,<dst_x>,<dst_y>,<kind>,<spread>,<x0>,<y0>,<x1>,<y1>,<n_stops> stops=<offset,r,g,b,a;...> |
//          clip=<x0,y0,x1,y1,sx,sy> tiles=<tx0,tiles_x,tiles_y,sx0,dst_vec,src_vec> c=<c0,c1,c2> table=<1024 x 8 hex digits>
// with "paint=null" for a NULL parameter block, "| nothing" for a valid call that launches nothing and "| err=<the message
// left>" for a refused one.  tests/test_layer_paint_tables.py restates the checks, the clipping, the coefficients and the
// table in Python from the inputs of each line and compares.  After each line it checks what the kernel relies on (the
// tiles cover the clipped rectangle from a multiple of four columns; the window's part lies inside the layer; the sum of t
// stays below 2^60 and the radial distances below 2^27 at the rectangle's corners) and fails with the case and the
// property on stderr.
#include "../csrc/fr_layer_paint_plan.hpp"
#include "selftest.hpp"

#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

using namespace selftest;

namespace {

struct Case {
    std::string name;
    uintptr_t src;
    size_t ss, sr;
    uintptr_t dst;
    size_t ds, dr;
    uint32_t flags;
    fr_layer_paint_params p;
    bool null_paint = false;
};

constexpr uintptr_t SRC = 0x10000000u, DST = 0x20000000u;
constexpr int32_t P26 = 1 << 26;

using Stops = std::vector<fr_gradient_stop>;
const Stops TWO = {{0, {255, 0, 0, 255}}, {65536, {0, 0, 255, 255}}};

fr_layer_paint_params P(uint32_t sx, uint32_t sy, uint32_t w, uint32_t h, int32_t dx, int32_t dy, uint32_t kind, uint32_t spread, int32_t x0, int32_t y0,
                        int32_t x1, int32_t y1, const Stops &stops = TWO)
{
    fr_layer_paint_params p{};
    p.src_x = sx, p.src_y = sy, p.w = w, p.h = h, p.dst_x = dx, p.dst_y = dy, p.kind = kind, p.spread = spread;
    p.x0 = x0, p.y0 = y0, p.x1 = x1, p.y1 = y1;
    p.n_stops = (uint32_t)stops.size();
    for (size_t i = 0; i < stops.size() && i < FR_GRADIENT_MAX_STOPS; ++i) p.stops[i] = stops[i];
    return p;
}
fr_layer_paint_params stops_n(fr_layer_paint_params p, uint32_t n) { p.n_stops = n; return p; }

// the layer is 300 x 40 and the image 300 x 40 (rows of 300 or 301) unless a case says otherwise
std::vector<Case> cases()
{
    const fr_layer_paint_params lin = P(0, 0, 300, 40, 0, 0, 0, 0, 0, 0, 300 * 64, 0), rad = P(0, 0, 300, 40, 0, 0, 1, 0, 150 * 64, 20 * 64, 100 * 64, 0);
    std::vector<Case> c;
    c.push_back({"linear_whole_image", SRC, 300, 40, DST, 300, 40, 0, lin});
    c.push_back({"radial_whole_image", SRC, 300, 40, DST, 300, 40, FR_LAYER_SRGB, rad});
    c.push_back({"no_layer", 0, 0, 0, DST, 300, 40, 0, lin});
    c.push_back({"no_layer_radial_reflect", 0, 0, 0, DST, 300, 40, 0, P(0, 0, 300, 40, 0, 0, 1, 2, 150 * 64 + 32, 20 * 64 + 32, 64, 0)});
    c.push_back({"margin", SRC, 300, 40, DST, 300, 40, 0, P(3, 2, 290, 35, 5, 3, 0, 1, 64, 64, 4160, 4160)});
    c.push_back({"rows301_no_vec", SRC, 300, 40, DST, 301, 40, 0, lin});
    c.push_back({"dst_4_aligned_only", SRC, 300, 40, DST + 4, 300, 40, 0, lin});
    c.push_back({"src_4_aligned_only", SRC + 4, 300, 40, DST, 300, 40, 0, lin});
    c.push_back({"window_off_the_grid", SRC, 300, 40, DST, 300, 40, 0, P(1, 0, 200, 40, 0, 0, 0, 0, 0, 0, 6400, 0)});
    c.push_back({"window_and_rectangle_off_alike", SRC, 300, 40, DST, 300, 40, 0, P(5, 0, 200, 40, 9, 0, 0, 0, 0, 0, 6400, 0)});
    c.push_back({"negative_position", SRC, 300, 40, DST, 300, 40, 0, P(0, 0, 300, 40, -7, -5, 0, 2, 100, 200, 9000, -3000)});
    c.push_back({"negative_position_window_at_1", SRC, 300, 40, DST, 300, 40, 0, P(1, 1, 299, 39, -2, -1, 1, 1, -6400, -6400, 6400, 0)});
    c.push_back({"over_the_right_and_bottom", SRC, 300, 40, DST, 300, 40, 0, P(0, 0, 300, 40, 200, 30, 0, 0, 64 * 200, 0, 64 * 300, 640)});
    c.push_back({"clipped_away_right", SRC, 300, 40, DST, 300, 40, 0, P(0, 0, 300, 40, 300, 0, 0, 0, 0, 0, 6400, 0)});
    c.push_back({"clipped_away_above", SRC, 300, 40, DST, 300, 40, 0, P(0, 0, 300, 40, 0, -40, 1, 0, 0, 0, 6400, 0)});
    c.push_back({"clipped_away_far", SRC, 300, 40, DST, 300, 40, 0, P(0, 0, 300, 40, INT32_MIN, INT32_MAX, 0, 0, 0, 0, 6400, 0)});
    c.push_back({"zero_width", SRC, 300, 40, DST, 300, 40, 0, P(0, 0, 0, 40, 0, 0, 0, 0, 0, 0, 6400, 0)});
    c.push_back({"zero_height_window_outside", SRC, 300, 40, DST, 300, 40, 0, P(500, 500, 40, 0, 0, 0, 0, 0, 0, 0, 6400, 0)});
    c.push_back({"one_stop", 0, 0, 0, DST, 300, 40, 0, P(0, 0, 300, 40, 0, 0, 0, 0, 0, 0, 6400, 0, {{30000, {9, 8, 7, 200}}})});
    c.push_back({"eight_stops", 0, 0, 0, DST, 300, 40, 0,
                 P(0, 0, 300, 40, 0, 0, 0, 0, 0, 0, 6400, 0, {{0, {255, 0, 0, 255}}, {100, {0, 255, 0, 0}}, {9000, {0, 0, 255, 255}}, {9000, {255, 255, 0, 128}},
                                                             {30001, {1, 2, 3, 4}}, {30002, {250, 251, 252, 253}}, {65535, {0, 0, 0, 0}}, {65536, {255, 255, 255, 255}}})});
    c.push_back({"hard_edges_only", 0, 0, 0, DST, 300, 40, 0, P(0, 0, 300, 40, 0, 0, 0, 0, 0, 0, 6400, 0, {{32768, {255, 0, 0, 255}}, {32768, {0, 255, 0, 255}}, {32768, {0, 0, 255, 77}}})});
    c.push_back({"stops_inside", 0, 0, 0, DST, 300, 40, 0, P(0, 0, 300, 40, 0, 0, 0, 0, 0, 0, 6400, 0, {{16000, {255, 0, 0, 255}}, {48031, {0, 0, 255, 0}}})});
    c.push_back({"shallow_angle", SRC, 300, 40, DST, 300, 40, 0, P(0, 0, 300, 40, 0, 0, 0, 0, 37, -11, 19001, 1733)});
    c.push_back({"reversed", SRC, 300, 40, DST, 300, 40, 0, P(0, 0, 300, 40, 0, 0, 0, 0, 300 * 64, 0, 0, 0)});
    c.push_back({"shortest_linear", SRC, 300, 40, DST, 300, 40, 0, P(0, 0, 300, 40, 0, 0, 0, 1, 0, 0, 64, 0)});
    c.push_back({"shortest_radial", SRC, 300, 40, DST, 300, 40, 0, P(0, 0, 300, 40, 0, 0, 1, 1, 0, 0, 64, 0)});
    c.push_back({"geometry_at_the_limit", SRC, 300, 40, DST, 300, 40, 0, P(0, 0, 300, 40, 0, 0, 0, 0, -P26, -P26, P26, P26)});
    // the last column whose ddx stays below 2^27 from a centre at -2^26 is 2^20 - 1
    c.push_back({"radial_centre_at_the_limit", SRC, 300, 2, (uintptr_t)1 << 40, (1 << 20) + 300, 2, 0, P(0, 0, 300, 2, (1 << 20) - 300, 0, 1, 1, -P26, 0, P26, 0)});
    c.push_back({"far_pixels_linear", SRC, 300, 2, (uintptr_t)1 << 40, (1 << 20) + 300, 2, 0, P(0, 0, 300, 2, 1 << 20, 0, 0, 1, 0, 0, 64, 0)});
    c.push_back({"pitch_max_last_columns", 0, 0, 0, (uintptr_t)1 << 40, (size_t)1 << 26, 3, 0, P(0, 0, 100, 3, P26 - 100, 0, 0, 2, P26, 0, -P26, 64)});
    c.push_back({"tiles_at_the_limit", 0, 0, 0, (uintptr_t)1 << 44, (size_t)1 << 16, (size_t)1 << 18, 0, P(0, 0, 1 << 16, 1 << 18, 0, 0, 0, 0, 0, 0, 6400, 0)});
    // every refusal, in the header's order
    c.push_back({"unknown_flag_2", SRC, 300, 40, DST, 300, 40, 2, lin});
    c.push_back({"text_flag_bits", SRC, 300, 40, DST, 300, 40, FR_TEXT_SRGB | FR_TEXT_OVER, lin});
    c.push_back({"dst_null", SRC, 300, 40, 0, 300, 40, 0, lin});
    c.push_back({"dst_not_4_aligned", SRC, 300, 40, DST + 2, 300, 40, 0, lin});
    c.push_back({"dst_pitch_over", SRC, 300, 40, DST, ((size_t)1 << 26) + 1, 40, 0, lin});
    c.push_back({"src_not_4_aligned", SRC + 1, 300, 40, DST, 300, 40, 0, lin});
    c.push_back({"src_pitch_over", SRC, ((size_t)1 << 26) + 1, 40, DST, 300, 40, 0, lin});
    c.push_back({"no_layer_with_stride", 0, 300, 0, DST, 300, 40, 0, lin});
    c.push_back({"no_layer_with_rows", 0, 0, 40, DST, 300, 40, 0, lin});
    c.push_back({"dst_rows_over", SRC, 300, 40, (uintptr_t)1 << 44, 4, (size_t)1 << 31, 0, lin});
    c.push_back({"src_rows_over", (uintptr_t)1 << 44, 4, (size_t)1 << 31, DST, 300, 40, 0, P(0, 0, 4, 40, 0, 0, 0, 0, 0, 0, 6400, 0)});
    c.push_back({"paint_null", SRC, 300, 40, DST, 300, 40, 0, lin, true});
    c.push_back({"window_leaves_right", SRC, 300, 40, DST, 300, 40, 0, P(1, 0, 300, 40, 0, 0, 0, 0, 0, 0, 6400, 0)});
    c.push_back({"window_leaves_below", SRC, 300, 40, DST, 300, 40, 0, P(0, 40, 300, 1, 0, 0, 0, 0, 0, 0, 6400, 0)});
    c.push_back({"window_wraps_uint32", SRC, 300, 40, DST, 300, 40, 0, P(UINT32_MAX, 0, 2, 2, 0, 0, 0, 0, 0, 0, 6400, 0)});
    c.push_back({"no_layer_with_src_x", 0, 0, 0, DST, 300, 40, 0, P(1, 0, 300, 40, 0, 0, 0, 0, 0, 0, 6400, 0)});
    c.push_back({"no_layer_with_src_y", 0, 0, 0, DST, 300, 40, 0, P(0, 1, 300, 40, 0, 0, 0, 0, 0, 0, 6400, 0)});
    c.push_back({"unknown_kind", SRC, 300, 40, DST, 300, 40, 0, P(0, 0, 300, 40, 0, 0, 2, 0, 0, 0, 6400, 0)});
    c.push_back({"unknown_spread", SRC, 300, 40, DST, 300, 40, 0, P(0, 0, 300, 40, 0, 0, 0, 3, 0, 0, 6400, 0)});
    c.push_back({"no_stops", SRC, 300, 40, DST, 300, 40, 0, stops_n(lin, 0)});
    c.push_back({"nine_stops", SRC, 300, 40, DST, 300, 40, 0, stops_n(lin, 9)});
    c.push_back({"offset_above_65536", SRC, 300, 40, DST, 300, 40, 0, P(0, 0, 300, 40, 0, 0, 0, 0, 0, 0, 6400, 0, {{0, {1, 2, 3, 4}}, {65537, {5, 6, 7, 8}}})});
    c.push_back({"offsets_decrease", SRC, 300, 40, DST, 300, 40, 0, P(0, 0, 300, 40, 0, 0, 0, 0, 0, 0, 6400, 0, {{0, {1, 2, 3, 4}}, {500, {5, 6, 7, 8}}, {499, {5, 6, 7, 8}}})});
    c.push_back({"linear_length_0", SRC, 300, 40, DST, 300, 40, 0, P(0, 0, 300, 40, 0, 0, 0, 0, 77, -5, 77, -5)});
    c.push_back({"radial_radius_0", SRC, 300, 40, DST, 300, 40, 0, P(0, 0, 300, 40, 0, 0, 1, 0, 0, 0, 0, 0)});
    c.push_back({"radial_radius_negative", SRC, 300, 40, DST, 300, 40, 0, P(0, 0, 300, 40, 0, 0, 1, 0, 0, 0, -6400, 0)});
    c.push_back({"radial_y1_set", SRC, 300, 40, DST, 300, 40, 0, P(0, 0, 300, 40, 0, 0, 1, 0, 0, 0, 6400, 1)});
    c.push_back({"images_overlap", DST + 4 * 300 * 39, 300, 40, DST, 300, 40, 0, lin});
    c.push_back({"images_adjoin", DST + 4 * 300 * 40, 300, 40, DST, 300, 40, 0, lin});
    c.push_back({"geometry_x0_over", SRC, 300, 40, DST, 300, 40, 0, P(0, 0, 300, 40, 0, 0, 0, 0, P26 + 1, 0, 0, 0)});
    c.push_back({"geometry_y0_under", SRC, 300, 40, DST, 300, 40, 0, P(0, 0, 300, 40, 0, 0, 1, 0, 0, -P26 - 1, 6400, 0)});
    c.push_back({"geometry_radius_over", SRC, 300, 40, DST, 300, 40, 0, P(0, 0, 300, 40, 0, 0, 1, 0, 0, 0, P26 + 1, 0)});
    c.push_back({"geometry_y1_over", SRC, 300, 40, DST, 300, 40, 0, P(0, 0, 300, 40, 0, 0, 0, 0, 0, 0, 0, INT32_MAX)});
    c.push_back({"linear_under_a_pixel", SRC, 300, 40, DST, 300, 40, 0, P(0, 0, 300, 40, 0, 0, 0, 0, 0, 0, 45, 45)});
    c.push_back({"linear_just_a_pixel", SRC, 300, 40, DST, 300, 40, 0, P(0, 0, 300, 40, 0, 0, 0, 0, 0, 0, 46, 45)});
    c.push_back({"radial_under_a_pixel", SRC, 300, 40, DST, 300, 40, 0, P(0, 0, 300, 40, 0, 0, 1, 0, 0, 0, 63, 0)});
    c.push_back({"radial_corner_too_far", SRC, 300, 2, (uintptr_t)1 << 40, (1 << 20) + 301, 2, 0, P(0, 0, 300, 2, (1 << 20) + 1, 0, 1, 1, -P26, 0, P26, 0)});
    c.push_back({"radial_too_far_but_clipped_away", SRC, 300, 2, (uintptr_t)1 << 40, (1 << 20) + 301, 2, 0, P(0, 0, 300, 2, (1 << 20) + 301, 0, 1, 1, -P26, 0, P26, 0)});
    c.push_back({"radial_row_too_far", 0, 0, 0, (uintptr_t)1 << 44, 4, (size_t)1 << 22, 0, P(0, 0, 4, 1 << 22, 0, 0, 1, 0, 0, -P26, 6400, 0)});
    c.push_back({"tiles_over", 0, 0, 0, (uintptr_t)1 << 44, (size_t)1 << 16, ((size_t)1 << 18) + 1, 0, P(0, 0, 1 << 16, (1 << 18) + 1, 0, 0, 0, 0, 0, 0, 6400, 0)});
    c.push_back({"tiles_over_by_the_lead", 0, 0, 0, (uintptr_t)1 << 44, ((size_t)1 << 16) + 4, (size_t)1 << 18, 0, P(0, 0, 1 << 16, 1 << 18, 1, 0, 0, 0, 0, 0, 6400, 0)});
    // the validation order, one case per rule: the earlier rule's code wins
    c.push_back({"order_flag_before_dst", SRC, 300, 40, 0, 300, 40, 2, lin});
    c.push_back({"order_dst_before_src", SRC + 1, 300, 40, DST + 1, 300, 40, 0, lin});
    c.push_back({"order_src_before_rows", SRC + 1, 300, 40, (uintptr_t)1 << 44, 4, (size_t)1 << 31, 0, lin});
    c.push_back({"order_rows_before_null_paint", SRC, 300, 40, (uintptr_t)1 << 44, 4, (size_t)1 << 31, 0, lin, true});
    c.push_back({"order_window_before_kind", SRC, 300, 40, DST, 300, 40, 0, P(1, 0, 300, 40, 0, 0, 7, 0, 0, 0, 6400, 0)});
    c.push_back({"order_kind_before_spread_before_stops", SRC, 300, 40, DST, 300, 40, 0, stops_n(P(0, 0, 300, 40, 0, 0, 7, 7, 0, 0, 6400, 0), 0)});
    c.push_back({"order_stops_before_length", SRC, 300, 40, DST, 300, 40, 0, stops_n(P(0, 0, 300, 40, 0, 0, 0, 0, 0, 0, 0, 0), 9)});
    c.push_back({"order_length_before_overlap", DST, 300, 40, DST, 300, 40, 0, P(0, 0, 300, 40, 0, 0, 0, 0, 5, 5, 5, 5)});
    c.push_back({"order_overlap_before_limits", DST, 300, 40, DST, 300, 40, 0, P(0, 0, 300, 40, 0, 0, 0, 0, 0, 0, P26 + 1, 0)});
    c.push_back({"order_limits_before_short", SRC, 300, 40, DST, 300, 40, 0, P(0, 0, 300, 40, 0, 0, 0, 0, P26 + 1, 0, P26 + 2, 0)});
    c.push_back({"order_short_before_corner", SRC, 300, 2, (uintptr_t)1 << 40, (1 << 20) + 301, 2, 0, P(0, 0, 300, 2, (1 << 20) + 1, 0, 1, 1, -P26, 0, 63, 0)});
    c.push_back({"refused_though_zero_size", SRC, 300, 40, DST, 300, 40, 0, P(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 6400, 0, {{9, {1, 2, 3, 4}}, {8, {5, 6, 7, 8}}})});
    return c;
}

// what the kernel relies on
void check_plan(const Case &cs, const fr::PaintPlan &t)
{
    const fr_layer_paint_params &p = cs.p;
    require(t.x0 < t.x1 && t.y0 < t.y1 && t.x1 <= cs.ds && t.y1 <= cs.dr, cs.name, "the clipped rectangle is empty or leaves the image");
    require(t.tx0 % fr::LAYER_LANE_PX == 0 && t.tx0 <= t.x0 && t.x0 - t.tx0 < fr::LAYER_LANE_PX, cs.name, "the first tile's column");
    require((uint64_t)t.tx0 + (uint64_t)fr::LAYER_TILE_W * t.tiles_x >= t.x1 && (uint64_t)t.tx0 + (uint64_t)fr::LAYER_TILE_W * (t.tiles_x - 1) < t.x1, cs.name,
            "the tile columns do not cover the rectangle exactly");
    require((uint64_t)t.y0 + (uint64_t)fr::LAYER_TILE_H * t.tiles_y >= t.y1 && (uint64_t)t.y0 + (uint64_t)fr::LAYER_TILE_H * (t.tiles_y - 1) < t.y1, cs.name,
            "the tile rows do not cover the rectangle exactly");
    require((uint64_t)t.tiles_x * t.tiles_y <= fr::LAYER_MAX_TILES, cs.name, "more tiles than a launch takes");
    require((int64_t)t.sx0 == (int64_t)t.sx - (int64_t)(t.x0 - t.tx0), cs.name, "the layer column of the first tile");
    if (cs.src) {
        require((uint64_t)t.sx + (t.x1 - t.x0) <= cs.ss && (uint64_t)t.sy + (t.y1 - t.y0) <= cs.sr, cs.name, "the window's part leaves the layer");
        require(t.sx >= p.src_x && t.sy >= p.src_y && (uint64_t)t.sx + (t.x1 - t.x0) <= (uint64_t)p.src_x + p.w && (uint64_t)t.sy + (t.y1 - t.y0) <= (uint64_t)p.src_y + p.h,
                cs.name, "the window's part leaves the window");
        if (t.src_vec) require(cs.src % 16 == 0 && cs.ss % 4 == 0 && (t.sx0 & 3) == 0, cs.name, "src_vec without 16-byte aligned groups");
    } else {
        require(!t.src_vec, cs.name, "src_vec without a layer");
    }
    if (t.dst_vec) require(cs.dst % 16 == 0 && cs.ds % 4 == 0, cs.name, "dst_vec without 16-byte aligned groups");
    for (const int64_t X : {(int64_t)t.x0, (int64_t)t.x1 - 1})
        for (const int64_t Y : {(int64_t)t.y0, (int64_t)t.y1 - 1}) {
            if (p.kind == FR_GRADIENT_RADIAL) {
                require(std::llabs(64 * X + 32 - p.x0) < fr::PAINT_MAX_DD && std::llabs(64 * Y + 32 - p.y0) < fr::PAINT_MAX_DD, cs.name, "a corner 2^27 or more from the centre");
            } else {
                const __int128 sum = (__int128)t.c[0] + (__int128)X * t.c[1] + (__int128)Y * t.c[2];
                require(sum < ((__int128)1 << 60) && sum > -((__int128)1 << 60), cs.name, "the sum of t reaches 2^60");
            }
        }
    if (p.kind == FR_GRADIENT_RADIAL) require(t.c[2] > 0 && t.c[2] <= ((int64_t)1 << 54), cs.name, "R beyond 2^54");
}

}  // namespace

int main()
{
    for (const Case &cs : cases()) {
        const fr::PaintIn in{cs.src, cs.dst, cs.ss, cs.sr, cs.ds, cs.dr, cs.null_paint ? nullptr : &cs.p, cs.flags};
        fr::PaintPlan t;
        clear_error();
        const int rc = fr::layer_paint_plan(in, t);
        const fr_layer_paint_params &p = cs.p;
        std::vector<std::string> sl;
        for (uint32_t i = 0; i < p.n_stops && i < FR_GRADIENT_MAX_STOPS; ++i)
            sl.push_back(fmt("%u,%u,%u,%u,%u", p.stops[i].offset, p.stops[i].rgba[0], p.stops[i].rgba[1], p.stops[i].rgba[2], p.stops[i].rgba[3]));
        printf("%s rc=%d in=%llu,%zu,%zu,%llu,%zu,%zu,%u ", cs.name.c_str(), rc, (unsigned long long)cs.src, cs.ss, cs.sr, (unsigned long long)cs.dst, cs.ds, cs.dr, cs.flags);
        if (cs.null_paint) printf("paint=null | ");
        else
            printf("paint=%u,%u,%u,%u,%d,%d,%u,%u,%d,%d,%d,%d,%u stops=%s | ", p.src_x, p.src_y, p.w, p.h, p.dst_x, p.dst_y, p.kind, p.spread, p.x0, p.y0, p.x1, p.y1, p.n_stops,
                   join(sl).c_str());
        if (rc) {
            printf("err=%s\n", last_error());
            continue;
        }
        if (t.nothing) {
            printf("nothing\n");
            continue;
        }
        printf("clip=%u,%u,%u,%u,%u,%u tiles=%u,%u,%u,%d,%d,%d c=%lld,%lld,%lld table=", t.x0, t.y0, t.x1, t.y1, t.sx, t.sy, t.tx0, t.tiles_x, t.tiles_y, t.sx0,
               t.dst_vec ? 1 : 0, t.src_vec ? 1 : 0, (long long)t.c[0], (long long)t.c[1], (long long)t.c[2]);
        for (uint32_t k = 0; k < fr::PAINT_TABLE; ++k) printf("%08x", t.table[k]);
        printf("\n");
        check_plan(cs, t);
    }
    return exit_status();
}

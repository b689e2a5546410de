// layer_warp_selftest.cpp — the host side of fr_layer_warp (csrc/fr_layer_warp_plan.cpp) on the CPU: links
// fr_layer_warp_plan.o and nothing else of the library.  No GPU; the device pointers are made-up integers.  It prints one
// line per case,
//   <case> rc=<code> in=<src>,<dst>,<src stride>,<src rows>,<dst stride>,<dst rows>,<flags>
//          blits=<sx,sy,w,h,dx,dy,dw,dh,u0,v0,ux,uy,vx,vy,o,reserved;...> | pixels=<n> walked=<n> opacity=<0|1>
//          clips=<x0,y0,x1,y1,X,Y;...> tiles=<x,y,x0,x1,y1,ov,wx,wy,U,V,ux,uy,vx,vy,ww,wh,i0,j0,i1,j1;...>
// or, for a refused call, "| err=<the message left>" behind the bar.  tests/test_layer_warp_tables.py restates the checks,
// the clipping, the culling and the tiles in Python from the inputs of each line and compares.  After the lines it checks
// the tables' own properties pixel by pixel (every pixel of a clipped rectangle that has a tap in its window lies in exactly
// one tile, whose origin reproduces its U and V and whose tap box holds those taps; no tile pixel outside its rectangle; a
// tap box inside the window; the vector flag only where the rows are on the 16-byte grid) and fails with the case and the
// property on stderr.
#include "../csrc/fr_layer_warp_plan.hpp"
#include "selftest.hpp"

#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

using namespace selftest;

namespace {

struct Case {
    std::string name;
    uintptr_t src, dst;
    size_t ss, sr, ds, dr;
    uint32_t flags;
    std::vector<fr_layer_warp_blit> blits;
    bool null_blits = false;
};

constexpr uintptr_t SRC = 0x10000000u, DST = 0x20000000u;
constexpr int32_t ONE = 65536, C45 = 46341, I31 = 0x7fffffff;
constexpr int64_t HALF = 32768, BIG = (int64_t)1 << 47;

fr_layer_warp_blit B(uint32_t sx, uint32_t sy, uint32_t w, uint32_t h, int32_t dx, int32_t dy, uint32_t dw, uint32_t dh, int64_t u0, int64_t v0, int32_t ux,
                     int32_t uy, int32_t vx, int32_t vy, uint32_t o = 255, uint32_t reserved = 0)
{
    return fr_layer_warp_blit{sx, sy, w, h, dx, dy, dw, dh, u0, v0, ux, uy, vx, vy, o, reserved};
}

// the layer is 70 x 50 and the image 300 x 200 unless a case says otherwise
std::vector<Case> cases()
{
    std::vector<Case> c;
    const fr_layer_warp_blit ok = B(0, 0, 70, 50, 0, 0, 70, 50, HALF, HALF, ONE, 0, 0, ONE);
    c.push_back({"identity_whole_layer", SRC, DST, 70, 50, 300, 200, 0, {ok}});
    c.push_back({"identity_srgb_at_an_offset", SRC, DST, 70, 50, 300, 200, FR_LAYER_SRGB, {B(0, 0, 70, 50, 13, 7, 70, 50, HALF, HALF, ONE, 0, 0, ONE, 200)}});
    c.push_back({"identity_window_inside", SRC, DST, 70, 50, 300, 200, 0, {B(9, 11, 37, 21, 30, 40, 37, 21, HALF, HALF, ONE, 0, 0, ONE)}});
    c.push_back({"identity_negative_offsets", SRC, DST, 70, 50, 301, 200, 0, {B(0, 0, 70, 50, -5, -7, 70, 50, HALF, HALF, ONE, 0, 0, ONE)}});
    c.push_back({"identity_partly_outside_right_bottom", SRC, DST, 70, 50, 300, 200, 0, {B(0, 0, 70, 50, 260, 170, 70, 50, HALF, HALF, ONE, 0, 0, ONE)}});
    c.push_back({"rectangle_one_larger_all_round", SRC, DST, 70, 50, 300, 200, 0, {B(0, 0, 70, 50, 9, 9, 72, 52, HALF - ONE, HALF - ONE, ONE, 0, 0, ONE)}});
    // a small window in a large rectangle: the culling
    c.push_back({"small_window_in_the_whole_image", SRC, DST, 70, 50, 300, 200, 0, {B(20, 20, 8, 8, 0, 0, 300, 200, HALF - 100 * ONE, HALF - 90 * ONE, ONE, 0, 0, ONE)}});
    c.push_back({"huge_rectangle_around_a_small_window", SRC, DST, 70, 50, 300, 200, 0,
                 {B(20, 20, 8, 8, -(1 << 19), -(1 << 19), 1u << 20, 1u << 20, HALF - ((int64_t)(1 << 19) + 150) * ONE, HALF - ((int64_t)(1 << 19) + 100) * ONE, ONE, 0, 0, ONE)}});
    c.push_back({"no_tap_reaches_the_window", SRC, DST, 70, 50, 300, 200, 0, {B(0, 0, 70, 50, 0, 0, 300, 200, HALF + 71 * (int64_t)ONE, HALF, ONE, 0, 0, ONE)}});
    c.push_back({"last_tap_column_reaches_the_window", SRC, DST, 70, 50, 300, 200, 0, {B(0, 0, 70, 50, 0, 0, 300, 200, HALF + 70 * (int64_t)ONE - 1, HALF, ONE, 0, 0, ONE)}});
    c.push_back({"first_tap_that_misses_on_the_left", SRC, DST, 70, 50, 300, 200, 0, {B(0, 0, 70, 50, 0, 0, 1, 1, -HALF - 1, HALF, 0, 0, 0, 0)}});
    c.push_back({"last_tap_that_hits_on_the_left", SRC, DST, 70, 50, 300, 200, 0, {B(0, 0, 70, 50, 0, 0, 1, 1, -HALF, HALF, 0, 0, 0, 0)}});
    c.push_back({"wholly_off_the_image", SRC, DST, 70, 50, 300, 200, 0, {B(0, 0, 70, 50, 300, 0, 70, 50, HALF, HALF, ONE, 0, 0, ONE)}});
    c.push_back({"wholly_off_the_image_by_min", SRC, DST, 70, 50, 300, 200, 0, {B(0, 0, 70, 50, INT32_MIN, INT32_MIN, 1u << 26, 1u << 26, HALF, HALF, ONE, 0, 0, ONE)}});
    c.push_back({"far_right_max", SRC, DST, 70, 50, 300, 200, 0, {B(0, 0, 70, 50, INT32_MAX, INT32_MAX, 1u << 26, 1u << 26, HALF, HALF, ONE, 0, 0, ONE)}});
    // turns, scales, mirrors
    c.push_back({"turned_45", SRC, DST, 70, 50, 300, 200, 0, {B(0, 0, 70, 50, 20, 10, 100, 100, -20 * (int64_t)ONE, 25 * (int64_t)ONE, C45, C45, -C45, C45)}});
    c.push_back({"turned_45_srgb_opacity", SRC, DST, 70, 50, 300, 200, FR_LAYER_SRGB, {B(0, 0, 70, 50, 20, 10, 100, 100, -20 * (int64_t)ONE, 25 * (int64_t)ONE, C45, C45, -C45, C45, 128)}});
    c.push_back({"turned_5_window_inside", SRC, DST, 70, 50, 300, 200, 0, {B(3, 4, 60, 40, 2, 3, 90, 70, -3 * (int64_t)ONE, 2 * (int64_t)ONE, 65287, 5712, -5712, 65287)}});
    c.push_back({"quarter_turn", SRC, DST, 70, 50, 300, 200, 0, {B(0, 0, 70, 50, 40, 20, 50, 70, HALF, HALF + 49 * (int64_t)ONE, 0, ONE, -ONE, 0)}});
    c.push_back({"mirrored", SRC, DST, 70, 50, 300, 200, 0, {B(0, 0, 70, 50, 40, 20, 70, 50, HALF + 69 * (int64_t)ONE, HALF, -ONE, 0, 0, ONE)}});
    c.push_back({"zoomed_2_5", SRC, DST, 70, 50, 300, 200, 0, {B(0, 0, 70, 50, 5, 5, 177, 127, 0, 0, 26214, 0, 0, 26214)}});
    c.push_back({"shrunk_0_4", SRC, DST, 70, 50, 300, 200, 0, {B(0, 0, 70, 50, 50, 50, 30, 22, 0, 0, 163840, 0, 0, 163840)}});
    c.push_back({"half_pixel_shift", SRC, DST, 70, 50, 300, 200, 0, {B(0, 0, 70, 50, 8, 8, 71, 50, 0, HALF, ONE, 0, 0, ONE)}});
    c.push_back({"zero_matrix_in_the_window", SRC, DST, 70, 50, 300, 200, 0, {B(0, 0, 70, 50, 10, 10, 40, 40, 5 * (int64_t)ONE + 77, 6 * (int64_t)ONE + 99, 0, 0, 0, 0)}});
    c.push_back({"zero_matrix_outside_the_window", SRC, DST, 70, 50, 300, 200, 0, {B(0, 0, 70, 50, 10, 10, 40, 40, -5 * (int64_t)ONE, 6 * (int64_t)ONE, 0, 0, 0, 0)}});
    // extremes
    c.push_back({"coefficients_max", SRC, DST, 70, 50, 300, 200, 0, {B(0, 0, 70, 50, 0, 0, 300, 200, HALF, HALF, I31, I31, I31, I31)}});
    c.push_back({"coefficients_min_plus_one", SRC, DST, 70, 50, 300, 200, 0, {B(0, 0, 70, 50, 0, 0, 300, 200, HALF + 69 * (int64_t)ONE, HALF + 49 * (int64_t)ONE, -I31, -I31, -I31, -I31)}});
    c.push_back({"coefficients_int32_min", SRC, DST, 70, 50, 300, 200, 0, {B(0, 0, 70, 50, 0, 0, 300, 200, HALF, HALF, INT32_MIN, INT32_MIN, INT32_MIN, INT32_MIN)}});
    c.push_back({"coefficients_max_over_the_largest_rectangle", SRC, DST, 70, 50, (size_t)1 << 26, 3, 0, {B(0, 0, 70, 50, 0, 0, 1u << 26, 1u << 26, BIG, -BIG, I31, I31, -I31, -I31)}});
    c.push_back({"origin_plus_2_47", SRC, DST, 70, 50, 300, 200, 0, {B(0, 0, 70, 50, 0, 0, 300, 200, BIG, HALF, -I31, 0, 0, ONE)}});
    c.push_back({"origin_minus_2_47_far_away", SRC, DST, 70, 50, 300, 200, 0, {B(0, 0, 70, 50, 0, 0, 300, 200, -BIG, -BIG, I31, 0, 0, I31)}});
    c.push_back({"origin_minus_2_47_walks_into_the_window", SRC, DST, 70, 50, ((size_t)1 << 17) + 4, 2, 0, {B(0, 0, 70, 50, 0, 0, (1u << 17) + 1, 2, -BIG, HALF, 1 << 30, 0, 0, ONE)}});
    c.push_back({"origin_over", SRC, DST, 70, 50, 300, 200, 0, {B(0, 0, 70, 50, 0, 0, 10, 10, BIG + 1, HALF, ONE, 0, 0, ONE)}});
    c.push_back({"origin_v_under", SRC, DST, 70, 50, 300, 200, 0, {B(0, 0, 70, 50, 0, 0, 10, 10, HALF, -BIG - 1, ONE, 0, 0, ONE)}});
    c.push_back({"rectangle_width_over", SRC, DST, 70, 50, 300, 200, 0, {B(0, 0, 70, 50, 0, 0, (1u << 26) + 1, 10, HALF, HALF, ONE, 0, 0, ONE)}});
    c.push_back({"rectangle_height_over", SRC, DST, 70, 50, 300, 200, 0, {B(0, 0, 70, 50, 0, 0, 10, (1u << 26) + 1, HALF, HALF, ONE, 0, 0, ONE)}});
    c.push_back({"rectangle_max", SRC, DST, 70, 50, 300, 200, 0, {B(0, 0, 70, 50, -5, -5, 1u << 26, 1u << 26, HALF - 5 * ONE, HALF - 5 * ONE, ONE, 0, 0, ONE)}});
    // empty things
    c.push_back({"zero_width_rectangle", SRC, DST, 70, 50, 300, 200, 0, {B(0, 0, 70, 50, 5, 5, 0, 9, HALF, HALF, ONE, 0, 0, ONE), B(0, 0, 70, 50, 5, 5, 9, 0, HALF, HALF, ONE, 0, 0, ONE)}});
    c.push_back({"zero_width_window", SRC, DST, 70, 50, 300, 200, 0, {B(70, 50, 0, 0, 5, 5, 20, 20, HALF, HALF, ONE, 0, 0, ONE), B(3, 3, 5, 0, 50, 5, 20, 20, HALF, HALF, ONE, 0, 0, ONE)}});
    c.push_back({"zero_width_window_out_of_the_layer", SRC, DST, 70, 50, 300, 200, 0, {B(71, 0, 0, 0, 5, 5, 20, 20, HALF, HALF, ONE, 0, 0, ONE)}});
    c.push_back({"opacity_0_has_no_tile", SRC, DST, 70, 50, 300, 200, 0, {B(0, 0, 70, 50, 0, 0, 70, 50, HALF, HALF, ONE, 0, 0, ONE, 0), B(0, 0, 70, 50, 100, 0, 70, 50, HALF, HALF, ONE, 0, 0, ONE)}});
    c.push_back({"all_opacity_0", SRC, DST, 70, 50, 300, 200, 0, {B(0, 0, 70, 50, 0, 0, 70, 50, HALF, HALF, ONE, 0, 0, ONE, 0)}});
    c.push_back({"opacity_instance_only_for_listed_tiles", SRC, DST, 70, 50, 300, 200, 0,
                 {B(0, 0, 70, 50, 0, 0, 70, 50, HALF, HALF, ONE, 0, 0, ONE), B(0, 0, 70, 50, 100, 0, 70, 50, HALF + 80 * (int64_t)ONE, HALF, ONE, 0, 0, ONE, 128)}});
    c.push_back({"no_blits", SRC, DST, 70, 50, 300, 200, 0, {}});
    // several blits; the overlap rule
    c.push_back({"touching_rectangles_with_their_own_maps", SRC, DST, 70, 50, 300, 200, FR_LAYER_SRGB,
                 {B(0, 0, 70, 50, 10, 10, 60, 60, 0, 0, C45, C45, -C45, C45, 255), B(0, 0, 70, 50, 70, 10, 60, 60, HALF, HALF, ONE, 0, 0, ONE, 128),
                  B(5, 5, 30, 30, 10, 70, 120, 33, 0, 0, 16384, 0, 0, 65536, 1), B(0, 0, 70, 50, 130, 10, 33, 93, HALF + 69 * (int64_t)ONE, HALF, -ONE, 0, 0, ONE, 77)}});
    c.push_back({"two_overlap_by_one_pixel", SRC, DST, 70, 50, 300, 200, 0, {B(0, 0, 70, 50, 10, 10, 20, 10, HALF, HALF, ONE, 0, 0, ONE), B(0, 0, 70, 50, 29, 19, 20, 10, HALF, HALF, ONE, 0, 0, ONE)}});
    c.push_back({"overlap_only_before_clipping", SRC, DST, 70, 50, 300, 200, 0, {B(0, 0, 70, 50, -30, 0, 20, 10, HALF, HALF, ONE, 0, 0, ONE), B(0, 0, 70, 50, -25, 5, 20, 10, HALF, HALF, ONE, 0, 0, ONE)}});
    c.push_back({"overlap_with_an_opacity_0_blit", SRC, DST, 70, 50, 300, 200, 0, {B(0, 0, 70, 50, 10, 10, 20, 10, HALF, HALF, ONE, 0, 0, ONE, 0), B(0, 0, 70, 50, 29, 19, 20, 10, HALF, HALF, ONE, 0, 0, ONE)}});
    c.push_back({"overlap_with_a_blit_no_tap_reaches", SRC, DST, 70, 50, 300, 200, 0, {B(0, 0, 70, 50, 10, 10, 20, 10, -BIG, HALF, 0, 0, 0, 0), B(0, 0, 70, 50, 29, 19, 20, 10, HALF, HALF, ONE, 0, 0, ONE)}});
    c.push_back({"overlap_names_the_first_pair", SRC, DST, 70, 50, 300, 200, 0,
                 {B(0, 0, 70, 50, 100, 140, 5, 5, HALF, HALF, ONE, 0, 0, ONE), B(0, 0, 70, 50, 10, 10, 20, 10, HALF, HALF, ONE, 0, 0, ONE), B(0, 0, 70, 50, 29, 19, 20, 10, HALF, HALF, ONE, 0, 0, ONE)}});
    // the window and the layer
    c.push_back({"window_one_pixel_out_right", SRC, DST, 70, 50, 300, 200, 0, {B(34, 0, 37, 21, 0, 0, 10, 10, HALF, HALF, ONE, 0, 0, ONE)}});
    c.push_back({"window_last_column_in", SRC, DST, 70, 50, 300, 200, 0, {B(33, 29, 37, 21, 0, 0, 40, 30, HALF, HALF, ONE, 0, 0, ONE)}});
    c.push_back({"window_one_row_out_below", SRC, DST, 70, 50, 300, 200, 0, {B(0, 30, 37, 21, 0, 0, 10, 10, HALF, HALF, ONE, 0, 0, ONE)}});
    c.push_back({"windows_1x1_1x9_9x1", SRC, DST, 70, 50, 300, 200, 0,
                 {B(5, 5, 1, 1, 0, 0, 5, 5, HALF - 2 * ONE + 16384, HALF - 2 * ONE + 16384, ONE, 0, 0, ONE), B(5, 5, 1, 9, 40, 0, 5, 13, HALF - 2 * ONE + 100, HALF - 2 * ONE, ONE, 0, 0, ONE),
                  B(5, 5, 9, 1, 80, 0, 13, 5, HALF - 2 * ONE, HALF - 2 * ONE + 65280, ONE, 0, 0, ONE)}});
    // pointers and pitches on and off their grids
    c.push_back({"dst_4_aligned_only", SRC, DST + 4, 70, 50, 300, 200, 0, {ok}});
    c.push_back({"dst_rows_off_the_grid", SRC, DST, 70, 50, 301, 200, 0, {ok}});
    c.push_back({"src_4_aligned_only_and_odd_pitch", SRC + 4, DST, 71, 50, 300, 200, 0, {ok}});
    for (int32_t dx = 0; dx < 4; ++dx)
        c.push_back({"dst_x_" + std::to_string(dx) + "_across_a_tile_border", SRC, DST, 70, 50, 300, 200, 0, {B(9, 11, 37, 21, 28 + dx, 25, 37, 21, HALF, HALF, ONE, 0, 0, ONE)}});
    // NULL pointers, flags, pitches, rows: the order of the checks
    c.push_back({"src_null", 0, DST, 70, 50, 300, 200, 0, {ok}});
    c.push_back({"dst_null", SRC, 0, 70, 50, 300, 200, 0, {ok}});
    c.push_back({"src_not_4_aligned", SRC + 2, DST, 70, 50, 300, 200, 0, {ok}});
    c.push_back({"dst_not_4_aligned", SRC, DST + 1, 70, 50, 300, 200, 0, {ok}});
    c.push_back({"blits_null", SRC, DST, 70, 50, 300, 200, 0, {ok}, true});
    for (uint32_t f : {(uint32_t)FR_LCD_BGR, (uint32_t)FR_MASK_PLANE, (uint32_t)FR_MASK_ERASE, 16u, (uint32_t)FR_TEXT_OVER, 1u << 31})
        c.push_back({"unknown_flag_" + std::to_string(f), SRC, DST, 70, 50, 300, 200, f, {ok}});
    c.push_back({"flag_comes_before_src", 0, DST, 70, 50, 300, 200, 2, {ok}});
    c.push_back({"src_comes_before_dst", SRC + 1, 0, 70, 50, 300, 200, 0, {ok}});
    c.push_back({"dst_comes_before_rows", SRC, DST + 1, 70, (size_t)1 << 31, 300, 200, 0, {ok}});
    c.push_back({"rows_come_before_blits", SRC, DST, 70, (size_t)1 << 31, 300, 200, 0, {ok}, true});
    c.push_back({"blits_come_before_aliasing", DST, DST, 300, 200, 300, 200, 0, {ok}, true});
    c.push_back({"aliasing_comes_before_opacity", DST, DST, 300, 200, 300, 200, 0, {B(0, 0, 70, 50, 0, 0, 70, 50, HALF, HALF, ONE, 0, 0, ONE, 256)}});
    c.push_back({"dst_in_the_layers_last_pixel", SRC, SRC + 4 * 70 * 50 - 4, 70, 50, 300, 200, 0, {ok}});
    c.push_back({"dst_behind_the_layer", SRC, SRC + 4 * 70 * 50, 70, 50, 300, 200, 0, {ok}});
    c.push_back({"opacity_256", SRC, DST, 70, 50, 300, 200, 0, {B(0, 0, 70, 50, 0, 0, 70, 50, HALF, HALF, ONE, 0, 0, ONE, 256)}});
    c.push_back({"reserved_1", SRC, DST, 70, 50, 300, 200, 0, {B(0, 0, 70, 50, 0, 0, 70, 50, HALF, HALF, ONE, 0, 0, ONE, 255, 1)}});
    c.push_back({"reserved_1_on_an_empty_blit", SRC, DST, 70, 50, 300, 200, 0, {B(0, 0, 70, 50, 0, 0, 0, 0, HALF, HALF, ONE, 0, 0, ONE, 255, 1)}});
    c.push_back({"opacity_comes_before_reserved", SRC, DST, 70, 50, 300, 200, 0, {B(0, 0, 70, 50, 0, 0, 70, 50, HALF, HALF, ONE, 0, 0, ONE, 256, 1)}});
    c.push_back({"reserved_comes_before_origin", SRC, DST, 70, 50, 300, 200, 0, {B(0, 0, 70, 50, 0, 0, 70, 50, BIG + 1, HALF, ONE, 0, 0, ONE, 255, 1)}});
    c.push_back({"origin_comes_before_rectangle", SRC, DST, 70, 50, 300, 200, 0, {B(0, 0, 70, 50, 0, 0, (1u << 26) + 1, 50, BIG + 1, HALF, ONE, 0, 0, ONE)}});
    c.push_back({"rectangle_comes_before_window", SRC, DST, 70, 50, 300, 200, 0, {B(1, 0, 70, 50, 0, 0, (1u << 26) + 1, 50, HALF, HALF, ONE, 0, 0, ONE)}});
    c.push_back({"window_comes_before_overlap", SRC, DST, 70, 50, 300, 200, 0,
                 {B(0, 0, 70, 50, 10, 10, 20, 10, HALF, HALF, ONE, 0, 0, ONE), B(0, 0, 70, 50, 29, 19, 20, 10, HALF, HALF, ONE, 0, 0, ONE), B(69, 0, 2, 2, 0, 0, 5, 5, HALF, HALF, ONE, 0, 0, ONE)}});
    c.push_back({"pitch_max", SRC, (uintptr_t)1 << 40, 70, 50, (size_t)1 << 26, 3, 0, {B(0, 0, 70, 50, (1 << 26) - 40, 0, 70, 50, HALF, HALF, ONE, 0, 0, ONE)}});
    c.push_back({"dst_pitch_over", SRC, (uintptr_t)1 << 40, 70, 50, ((size_t)1 << 26) + 1, 3, 0, {ok}});
    c.push_back({"src_pitch_over", SRC, (uintptr_t)1 << 40, ((size_t)1 << 26) + 1, 3, 300, 200, 0, {ok}});
    c.push_back({"dst_rows_over", SRC, (uintptr_t)1 << 40, 70, 50, 4, (size_t)1 << 31, 0, {ok}});
    c.push_back({"src_rows_over", (uintptr_t)1 << 44, DST, 4, (size_t)1 << 31, 300, 200, 0, {ok}});
    c.push_back({"tall_image_last_rows", SRC, (uintptr_t)1 << 44, 70, 50, 4, 0x7fffffffu, 0, {B(0, 0, 70, 50, 0, 0x7fffffff - 20, 4, 50, HALF, HALF, ONE, 0, 0, ONE, 77)}});
    c.push_back({"too_many_tiles", SRC, (uintptr_t)1 << 40, 70, 50, (size_t)1 << 26, (size_t)1 << 11, 0, {B(0, 0, 70, 50, 0, 0, 1u << 26, 1u << 11, HALF, HALF, ONE, 0, 0, ONE)}});
    c.push_back({"as_many_tiles_as_allowed", SRC, (uintptr_t)1 << 40, 70, 50, (size_t)1 << 16, (size_t)1 << 16, 0, {B(0, 0, 70, 50, 0, 0, 1u << 16, 1u << 16, HALF, HALF, ONE, 0, 0, ONE)}});
    c.push_back({"too_many_tiles_counts_no_opacity_0_blit", SRC, (uintptr_t)1 << 40, 70, 50, (size_t)1 << 26, (size_t)1 << 11, 0,
                 {B(0, 0, 70, 50, 0, 0, 1u << 26, 1u << 11, HALF, HALF, ONE, 0, 0, ONE, 0)}});
    return c;
}

// the properties the kernel relies on, for small images: pixel by pixel
void check_tables(const Case &cs, const fr::WarpTables &t)
{
    for (const fr::WarpTile &tl : t.tiles) {
        require(tl.x % fr::LAYER_LANE_PX == 0, cs.name, "a tile's x is no multiple of the lane's pixels");
        require((tl.ov & 0xffu) != 0 && tl.ww && tl.wh, cs.name, "a tile of a blit that draws nothing");
        require(tl.i0 <= tl.i1 && tl.i1 < tl.ww && tl.j0 <= tl.j1 && tl.j1 < tl.wh, cs.name, "a tap box that is empty or leaves the window");
        require((uint64_t)tl.wx + tl.ww <= cs.ss && (uint64_t)tl.wy + tl.wh <= cs.sr, cs.name, "a window that leaves the layer");
        require(tl.y < tl.y1 && std::max(tl.x, tl.x0) < std::min(tl.x + fr::WARP_TILE, tl.x1), cs.name, "a tile without a pixel");
        if (tl.ov & fr::LAYER_DST_VEC) require((cs.dst + 4 * ((uint64_t)tl.y * cs.ds + tl.x)) % 16 == 0 && cs.ds % 4 == 0, cs.name, "LAYER_DST_VEC on unaligned rows");
    }
    if (cs.ds * cs.dr > ((size_t)1 << 20)) return;
    std::vector<int32_t> owner(cs.ds * cs.dr, -1);
    for (size_t k = 0; k < t.tiles.size(); ++k) {
        const fr::WarpTile &tl = t.tiles[k];
        for (uint32_t y = tl.y; y < tl.y + fr::WARP_TILE && y < tl.y1; ++y)
            for (uint32_t x = std::max(tl.x, tl.x0); x < tl.x + fr::WARP_TILE && x < tl.x1; ++x) {
                require(y < cs.dr && x < cs.ds, cs.name, "a tile pixel outside the destination");
                if (y >= cs.dr || x >= cs.ds) continue;
                require(owner[(size_t)y * cs.ds + x] < 0, cs.name, "a pixel in two tiles");
                owner[(size_t)y * cs.ds + x] = (int32_t)k;
            }
    }
    std::vector<uint8_t> count(cs.ds * cs.dr, 0);
    for (size_t b = 0; b < t.clips.size(); ++b) {
        const fr::LayerClip &c = t.clips[b];
        const fr_layer_warp_blit &bl = cs.blits[b];
        require(c.x0 >= c.x1 || (c.sx == (int64_t)c.x0 - bl.dst_x && c.sy == (int64_t)c.y0 - bl.dst_y), cs.name, "a clip's rectangle pixel");
        for (uint32_t y = c.y0; y < c.y1; ++y)
            for (uint32_t x = c.x0; x < c.x1; ++x) {
                require(++count[(size_t)y * cs.ds + x] == 1, cs.name, "clipped rectangles overlap");
                const int64_t X = (int64_t)x - bl.dst_x, Y = (int64_t)y - bl.dst_y;
                const int64_t U = bl.u0 + X * bl.ux + Y * bl.uy, V = bl.v0 + X * bl.vx + Y * bl.vy;
                const int64_t i = (U - HALF) >> 16, j = (V - HALF) >> 16;
                const bool ci[2] = {i >= 0 && i < (int64_t)bl.w, i + 1 >= 0 && i + 1 < (int64_t)bl.w}, cj[2] = {j >= 0 && j < (int64_t)bl.h, j + 1 >= 0 && j + 1 < (int64_t)bl.h};
                const bool hit = bl.opacity && (ci[0] || ci[1]) && (cj[0] || cj[1]);
                const int32_t k = owner[(size_t)y * cs.ds + x];
                if (!hit) continue;                             // (a pixel without a tap may still lie in a listed tile)
                require(k >= 0, cs.name, "a pixel with a tap in its window lies in no tile");
                if (k < 0) continue;
                const fr::WarpTile &tl = t.tiles[(size_t)k];
                require(tl.x0 == c.x0 && tl.x1 == c.x1 && tl.y1 == c.y1 && (tl.ov & 0xffu) == bl.opacity, cs.name, "a pixel in another blit's tile");
                require(tl.U + (int64_t)(x - tl.x) * tl.ux + (int64_t)(y - tl.y) * tl.uy == U && tl.V + (int64_t)(x - tl.x) * tl.vx + (int64_t)(y - tl.y) * tl.vy == V, cs.name,
                        "a tile's origin does not reproduce U and V");
                for (int a = 0; a < 2; ++a) {
                    if (ci[a]) require(i + a >= (int64_t)tl.i0 && i + a <= (int64_t)tl.i1, cs.name, "a tap column outside the tile's box");
                    if (cj[a]) require(j + a >= (int64_t)tl.j0 && j + a <= (int64_t)tl.j1, cs.name, "a tap row outside the tile's box");
                }
            }
    }
}

}  // namespace

int main()
{
    for (const Case &cs : cases()) {
        const fr::WarpIn in{cs.src, cs.dst, cs.ss, cs.sr, cs.ds, cs.dr, cs.null_blits ? nullptr : cs.blits.data(), (uint32_t)cs.blits.size(), cs.flags};
        fr::WarpTables t;
        clear_error();
        const int rc = fr::layer_warp_tables(in, t);
        std::vector<std::string> bl, cl, tl;
        for (const fr_layer_warp_blit &b : cs.blits)
            bl.push_back(fmt("%u,%u,%u,%u,%d,%d,%u,%u,%lld,%lld,%d,%d,%d,%d,%u,%u", b.src_x, b.src_y, b.w, b.h, b.dst_x, b.dst_y, b.dst_w, b.dst_h, (long long)b.u0, (long long)b.v0,
                         b.ux, b.uy, b.vx, b.vy, b.opacity, b.reserved));
        printf("%s rc=%d in=%llu,%llu,%zu,%zu,%zu,%zu,%u blits=%s%s | ", cs.name.c_str(), rc, (unsigned long long)cs.src, (unsigned long long)cs.dst, cs.ss, cs.sr, cs.ds, cs.dr,
               cs.flags, join(bl).c_str(), cs.null_blits ? " null" : "");
        if (rc) {
            printf("err=%s\n", last_error());
            continue;
        }
        for (const fr::LayerClip &c : t.clips) cl.push_back(fmt("%u,%u,%u,%u,%u,%u", c.x0, c.y0, c.x1, c.y1, c.sx, c.sy));
        for (const fr::WarpTile &x : t.tiles)
            tl.push_back(fmt("%u,%u,%u,%u,%u,%u,%u,%u,%lld,%lld,%d,%d,%d,%d,%u,%u,%u,%u,%u,%u", x.x, x.y, x.x0, x.x1, x.y1, x.ov, x.wx, x.wy, (long long)x.U, (long long)x.V, x.ux, x.uy,
                         x.vx, x.vy, x.ww, x.wh, x.i0, x.j0, x.i1, x.j1));
        printf("pixels=%llu walked=%llu opacity=%d clips=%s tiles=%s\n", (unsigned long long)t.pixels, (unsigned long long)t.walked, t.opacity ? 1 : 0, join(cl).c_str(),
               join(tl).c_str());
        check_tables(cs, t);
    }
    return exit_status();
}

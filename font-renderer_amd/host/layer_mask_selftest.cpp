// layer_mask_selftest.cpp — the host side of fr_layer_mask (csrc/fr_layer_mask_plan.cpp) on the CPU: links
// fr_layer_mask_plan.o and nothing else of the library.  No GPU; the device pointers are made-up integers.  It prints one
// line per case,
//   <case> rc=<code> in=<src>,<mask>,<dst>,<src stride>,<src rows>,<mask stride>,<mask rows>,<dst stride>,<dst rows>,<flags>
//          blits=<sx,sy,w,h,dx,dy,mx,my,o,invert;...> | pixels=<n> clips=<x0,y0,x1,y1,sx,sy;...> origins=<mx,my;...>
//          tiles=<x,y,x0,x1,y1,sx,sy,ov,mx,my,invert;...>
// or, for a refused call, "| err=<the message left>" behind the bar.  tests/test_layer_mask_tables.py restates the checks,
// the clipping and the tiling in Python from the inputs of each line and compares.  After the lines it checks the tables'
// own properties (every pixel of a clipped rectangle in exactly one tile, no tile pixel outside it or reading outside the
// layer or the mask, the vector flags only where the addresses are on their grids) and fails with the case and the property
// on stderr.
#include "../csrc/fr_layer_mask_plan.hpp"
#include "selftest.hpp"

#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

using namespace selftest;

namespace {

struct Case {
    std::string name;
    uintptr_t src, mask, dst;
    size_t ss, sr, ms, mr, ds, dr;
    uint32_t flags;
    std::vector<fr_layer_mask_blit> blits;
    bool null_blits = false;
};

constexpr uintptr_t SRC = 0x10000000u, MASK = 0x18000000u, DST = 0x20000000u;
constexpr uint32_t P = FR_MASK_PLANE, E = FR_MASK_ERASE, S = FR_LAYER_SRGB;

// the layer is 300 x 50 and the mask 320 x 60 unless a case says otherwise; the image 50 rows of 131 or 132 pixels
std::vector<Case> cases()
{
    std::vector<Case> c;
    const fr_layer_mask_blit ok{0, 0, 10, 10, 0, 0, 0, 0, 255, 0};
    c.push_back({"whole_layer_aligned", SRC, MASK, DST, 128, 40, 128, 40, 132, 50, 0, {{0, 0, 128, 40, 0, 0, 0, 0, 255, 0}}});
    c.push_back({"whole_plane_aligned", SRC, MASK, DST, 128, 40, 128, 40, 132, 50, P, {{0, 0, 128, 40, 0, 0, 0, 0, 255, 0}}});
    c.push_back({"erase_plane_aligned", 0, MASK, DST, 0, 0, 128, 40, 132, 50, P | E, {{0, 0, 128, 40, 0, 0, 0, 0, 255, 0}}});
    c.push_back({"erase_layer_mask_srgb", 0, MASK, DST, 0, 0, 128, 40, 132, 50, E | S, {{7, 9, 128, 40, 4, 0, 0, 0, 200, 1}}});
    c.push_back({"erase_ignores_src_xy_and_size", 0, MASK, DST, 1, (size_t)1 << 40, 128, 40, 132, 50, E, {{1000, 1000, 30, 20, -3, -4, 5, 6, 255, 0}}});
    c.push_back({"negative_offsets", SRC, MASK, DST, 300, 50, 320, 60, 131, 50, 0, {{0, 0, 97, 41, -5, -7, 2, 3, 255, 0}}});
    c.push_back({"negative_offsets_aligned_rows", SRC, MASK, DST, 300, 50, 320, 60, 132, 50, 0, {{0, 0, 97, 41, -5, -7, 3, 3, 255, 1}}});
    c.push_back({"partly_outside_right_bottom", SRC, MASK, DST, 300, 50, 320, 60, 132, 50, 0, {{3, 2, 97, 41, 100, 30, 11, 12, 255, 0}}});
    c.push_back({"wholly_outside_right", SRC, MASK, DST, 300, 50, 320, 60, 132, 50, 0, {{0, 0, 10, 10, 132, 0, 0, 0, 255, 0}}});
    c.push_back({"wholly_outside_above", SRC, MASK, DST, 300, 50, 320, 60, 132, 50, 0, {{0, 0, 10, 10, 5, -10, 0, 0, 255, 0}}});
    c.push_back({"wholly_outside_left_by_min", SRC, MASK, DST, 300, 50, 320, 60, 132, 50, 0, {{0, 0, 10, 10, INT32_MIN, INT32_MIN, 0, 0, 255, 0}}});
    c.push_back({"far_right_max", SRC, MASK, DST, 300, 50, 320, 60, 132, 50, P, {{0, 0, 10, 10, INT32_MAX, INT32_MAX, 0, 0, 255, 0}}});
    for (uint32_t w : {1u, 3u, 64u, 257u}) {
        c.push_back({"width_" + std::to_string(w), SRC, MASK, DST, 300, 50, 320, 60, 512, 50, 0, {{0, 0, w, 5, 8, 1, 4, 0, 255, 0}}});
        c.push_back({"width_" + std::to_string(w) + "_at_x3", SRC, MASK, DST, 300, 50, 320, 60, 512, 50, P, {{1, 0, w, 17, 3, 1, 2, 1, 255, 0}}});
    }
    c.push_back({"multi_blit", SRC, MASK, DST, 300, 50, 320, 60, 132, 50, S,
                 {{0, 0, 20, 10, 10, 10, 0, 0, 255, 0}, {20, 0, 20, 10, 30, 10, 5, 5, 128, 1}, {0, 10, 40, 5, 10, 20, 8, 8, 1, 0}, {0, 0, 30, 12, 0, 30, 0, 0, 0, 1},
                  {3, 3, 0, 9, 0, 0, 900, 900, 255, 0}, {40, 0, 57, 41, 60, 5, 260, 19, 254, 1}}});
    c.push_back({"two_overlap_by_one_pixel", SRC, MASK, DST, 300, 50, 320, 60, 132, 50, 0, {{0, 0, 20, 10, 10, 10, 0, 0, 255, 0}, {20, 0, 20, 10, 29, 19, 0, 0, 255, 0}}});
    c.push_back({"overlap_only_before_clipping", SRC, MASK, DST, 300, 50, 320, 60, 132, 50, 0, {{0, 0, 20, 10, -30, 0, 0, 0, 255, 0}, {0, 0, 20, 10, -25, 5, 0, 0, 255, 0}}});
    c.push_back({"overlap_with_an_opacity_0_blit", SRC, MASK, DST, 300, 50, 320, 60, 132, 50, P, {{0, 0, 20, 10, 10, 10, 0, 0, 0, 0}, {20, 0, 20, 10, 29, 19, 0, 0, 255, 0}}});
    c.push_back({"overlap_names_the_first_pair", SRC, MASK, DST, 300, 50, 320, 60, 132, 50, 0,
                 {{0, 0, 5, 5, 100, 40, 0, 0, 255, 0}, {0, 0, 20, 10, 10, 10, 0, 0, 255, 0}, {20, 0, 20, 10, 29, 19, 0, 0, 255, 0}}});
    c.push_back({"source_one_pixel_out_right", SRC, MASK, DST, 300, 50, 320, 60, 132, 50, 0, {{204, 0, 97, 41, 0, 0, 0, 0, 255, 0}}});
    c.push_back({"source_last_column_in", SRC, MASK, DST, 300, 50, 320, 60, 132, 50, 0, {{203, 9, 97, 41, 0, 0, 223, 19, 255, 0}}});
    c.push_back({"source_one_pixel_out_below", SRC, MASK, DST, 300, 50, 320, 60, 132, 50, 0, {{0, 10, 97, 41, 0, 0, 0, 0, 255, 0}}});
    c.push_back({"mask_one_element_out_right", SRC, MASK, DST, 300, 50, 320, 60, 132, 50, 0, {{0, 0, 97, 41, 0, 0, 224, 0, 255, 0}}});
    c.push_back({"mask_one_row_out_below", SRC, MASK, DST, 300, 50, 320, 60, 132, 50, P, {{0, 0, 97, 41, 0, 0, 0, 20, 255, 0}}});
    c.push_back({"mask_out_when_erasing", 0, MASK, DST, 0, 0, 320, 60, 132, 50, E, {{0, 0, 97, 41, 0, 0, 224, 0, 255, 0}}});
    c.push_back({"layer_out_comes_before_mask_out", SRC, MASK, DST, 300, 50, 320, 60, 132, 50, 0, {{204, 0, 97, 41, 0, 0, 224, 0, 255, 0}}});
    c.push_back({"opacity_256", SRC, MASK, DST, 300, 50, 320, 60, 132, 50, 0, {{0, 0, 10, 10, 0, 0, 0, 0, 256, 0}}});
    c.push_back({"invert_2", SRC, MASK, DST, 300, 50, 320, 60, 132, 50, 0, {{0, 0, 10, 10, 0, 0, 0, 0, 255, 2}}});
    c.push_back({"opacity_comes_before_invert", SRC, MASK, DST, 300, 50, 320, 60, 132, 50, 0, {{0, 0, 10, 10, 0, 0, 0, 0, 256, 2}}});
    c.push_back({"invert_2_on_an_empty_blit", SRC, MASK, DST, 300, 50, 320, 60, 132, 50, 0, {{0, 0, 0, 10, 0, 0, 0, 0, 255, 2}}});
    c.push_back({"invert_comes_before_leaving", SRC, MASK, DST, 300, 50, 320, 60, 132, 50, 0, {{299, 0, 10, 10, 0, 0, 0, 0, 255, 7}}});
    c.push_back({"opacity_0_has_no_tile", SRC, MASK, DST, 300, 50, 320, 60, 132, 50, 0, {{0, 0, 10, 10, 0, 0, 0, 0, 0, 0}, {0, 0, 10, 10, 20, 0, 0, 0, 255, 0}}});
    c.push_back({"all_opacity_0", SRC, MASK, DST, 300, 50, 320, 60, 132, 50, 0, {{0, 0, 10, 10, 0, 0, 0, 0, 0, 0}, {0, 0, 10, 10, 20, 0, 0, 0, 0, 1}}});
    c.push_back({"zero_width_anywhere", SRC, MASK, DST, 300, 50, 320, 60, 132, 50, 0, {{1000, 1000, 0, 7, 0, 0, 1000, 1000, 255, 0}, {0, 0, 7, 0, 0, 0, 0, 0, 255, 1}}});
    // what may alias and what may not
    c.push_back({"layer_and_mask_the_same_image", SRC, SRC, DST, 300, 50, 300, 50, 132, 50, 0, {ok}});
    c.push_back({"layer_and_plane_overlap", SRC, SRC + 77, DST, 300, 50, 300, 50, 132, 50, P, {ok}});
    c.push_back({"dst_is_the_layer", SRC, MASK, SRC, 300, 50, 320, 60, 300, 50, 0, {ok}});
    c.push_back({"dst_is_the_mask", SRC, MASK, MASK, 300, 50, 320, 60, 320, 60, 0, {ok}});
    c.push_back({"dst_is_the_mask_when_erasing", 0, MASK, MASK, 0, 0, 320, 60, 320, 60, E, {ok}});
    c.push_back({"dst_in_the_masks_last_byte", SRC, MASK, MASK + 4 * 320 * 60 - 4, 300, 50, 320, 60, 132, 50, 0, {ok}});
    c.push_back({"dst_behind_the_mask", SRC, MASK, MASK + 4 * 320 * 60, 300, 50, 320, 60, 132, 50, 0, {ok}});
    c.push_back({"dst_in_the_planes_last_bytes", SRC, MASK, MASK + 320 * 60 - 4, 300, 50, 320, 60, 132, 50, P, {ok}});
    c.push_back({"dst_behind_the_plane", SRC, MASK, MASK + 320 * 60, 300, 50, 320, 60, 132, 50, P, {ok}});
    c.push_back({"plane_ends_at_dst", SRC, DST - 320 * 60, DST, 300, 50, 320, 60, 132, 50, P, {ok}});
    c.push_back({"layer_overlap_comes_before_mask_overlap", DST, DST, DST, 132, 50, 132, 50, 132, 50, 0, {ok}});
    // pointers and pitches on and off their grids
    c.push_back({"src_not_4_aligned", SRC + 2, MASK, DST, 300, 50, 320, 60, 132, 50, 0, {ok}});
    c.push_back({"mask_not_4_aligned", SRC, MASK + 2, DST, 300, 50, 320, 60, 132, 50, 0, {ok}});
    c.push_back({"dst_not_4_aligned", SRC, MASK, DST + 1, 300, 50, 320, 60, 132, 50, 0, {ok}});
    c.push_back({"dst_4_aligned_only", SRC, MASK, DST + 4, 300, 50, 320, 60, 132, 50, 0, {{0, 0, 40, 10, 0, 0, 0, 0, 255, 0}}});
    c.push_back({"src_4_aligned_only", SRC + 8, MASK, DST, 300, 50, 320, 60, 132, 50, 0, {{0, 0, 40, 10, 0, 0, 0, 0, 255, 0}}});
    c.push_back({"mask_4_aligned_only", SRC, MASK + 12, DST, 300, 50, 320, 60, 132, 50, 0, {{0, 0, 40, 10, 0, 0, 0, 0, 255, 0}}});
    c.push_back({"mask_rows_off_the_grid", SRC, MASK, DST, 300, 50, 321, 60, 132, 50, 0, {{0, 0, 40, 10, 0, 0, 0, 0, 255, 0}}});
    c.push_back({"src_rows_off_the_grid", SRC, MASK, DST, 301, 50, 320, 60, 132, 50, 0, {{0, 0, 40, 10, 0, 0, 0, 0, 255, 0}}});
    c.push_back({"src_x_unaligned", SRC, MASK, DST, 300, 50, 320, 60, 132, 50, 0, {{5, 0, 40, 10, 8, 0, 4, 0, 255, 0}}});
    c.push_back({"mask_x_unaligned", SRC, MASK, DST, 300, 50, 320, 60, 132, 50, 0, {{4, 0, 40, 10, 8, 0, 5, 0, 255, 0}}});
    c.push_back({"all_match_dst_x_mod_4", SRC, MASK, DST, 300, 50, 320, 60, 132, 50, 0, {{6, 0, 40, 10, 10, 0, 14, 3, 255, 0}}});
    for (uint32_t off = 0; off < 4; ++off)
        for (uint32_t pitch = 320; pitch < 324; ++pitch)
            c.push_back({"plane_at_" + std::to_string(off) + "_pitch_" + std::to_string(pitch), SRC, MASK + off, DST, 300, 50, pitch, 60, 132, 50, P,
                         {{0, 0, 40, 10, 8, 0, 0, 2, 255, 0}, {0, 0, 40, 10, 12, 20, 4 - off, 0, 255, 0}}});
    c.push_back({"plane_pointer_plus_column_on_the_grid", SRC, MASK + 3, DST, 300, 50, 320, 60, 132, 50, P, {{0, 0, 40, 10, 8, 0, 1, 0, 255, 0}}});
    c.push_back({"plane_odd_pointer_is_valid", SRC, MASK + 1, DST, 300, 50, 317, 60, 131, 50, P | S, {{0, 0, 97, 41, -5, -7, 3, 3, 77, 1}}});
    // NULL pointers, flags, pitches, rows: the order of the checks
    c.push_back({"src_null", 0, MASK, DST, 300, 50, 320, 60, 132, 50, 0, {ok}});
    c.push_back({"mask_null", SRC, 0, DST, 300, 50, 320, 60, 132, 50, 0, {ok}});
    c.push_back({"plane_null", SRC, 0, DST, 300, 50, 320, 60, 132, 50, P, {ok}});
    c.push_back({"dst_null", SRC, MASK, 0, 300, 50, 320, 60, 132, 50, 0, {ok}});
    c.push_back({"erase_with_a_src", SRC, MASK, DST, 300, 50, 320, 60, 132, 50, E, {ok}});
    c.push_back({"erase_with_a_misaligned_src", SRC + 1, MASK, DST, 300, 50, 320, 60, 132, 50, E, {ok}});
    c.push_back({"blits_null", SRC, MASK, DST, 300, 50, 320, 60, 132, 50, 0, {ok}, true});
    c.push_back({"no_blits", SRC, MASK, DST, 300, 50, 320, 60, 132, 50, 0, {}});
    c.push_back({"unknown_flag_lcd_bgr", SRC, MASK, DST, 300, 50, 320, 60, 132, 50, FR_LCD_BGR, {ok}});
    c.push_back({"unknown_flag_16", SRC, MASK, DST, 300, 50, 320, 60, 132, 50, 16, {ok}});
    c.push_back({"text_flag_bits", SRC, MASK, DST, 300, 50, 320, 60, 132, 50, FR_TEXT_OVER, {ok}});
    c.push_back({"flag_comes_before_dst", SRC, MASK, 0, 300, 50, 320, 60, 132, 50, 2, {ok}});
    c.push_back({"dst_comes_before_mask", SRC, 0, DST + 1, 300, 50, 320, 60, 132, 50, 0, {ok}});
    c.push_back({"mask_comes_before_src", 0, MASK + 1, DST, 300, 50, 320, 60, 132, 50, 0, {ok}});
    c.push_back({"mask_comes_before_erase_src", SRC, 0, DST, 300, 50, 320, 60, 132, 50, E, {ok}});
    c.push_back({"src_comes_before_rows", SRC + 1, MASK, DST, 300, 50, 320, (size_t)1 << 31, 132, 50, 0, {ok}});
    c.push_back({"rows_come_before_blits", SRC, MASK, DST, 300, 50, 320, (size_t)1 << 31, 132, 50, 0, {ok}, true});
    c.push_back({"blits_come_before_aliasing", DST, MASK, DST, 132, 50, 320, 60, 132, 50, 0, {ok}, true});
    c.push_back({"aliasing_comes_before_opacity", DST, MASK, DST, 132, 50, 320, 60, 132, 50, 0, {{0, 0, 10, 10, 0, 0, 0, 0, 256, 0}}});
    c.push_back({"leaving_comes_before_overlap", SRC, MASK, DST, 300, 50, 320, 60, 132, 50, 0, {{0, 0, 20, 10, 10, 10, 0, 0, 255, 0}, {20, 0, 20, 10, 29, 19, 0, 0, 255, 0}, {299, 0, 2, 2, 0, 0, 0, 0, 255, 0}}});
    c.push_back({"pitch_max", SRC, MASK, (uintptr_t)1 << 40, 300, 50, (size_t)1 << 26, 3, (size_t)1 << 26, 3, P, {{0, 0, 300, 3, (1 << 26) - 100, 0, (1u << 26) - 300, 0, 255, 0}}});
    c.push_back({"dst_pitch_over", SRC, MASK, (uintptr_t)1 << 40, 300, 50, 320, 60, ((size_t)1 << 26) + 1, 3, 0, {ok}});
    c.push_back({"mask_pitch_over", SRC, MASK, (uintptr_t)1 << 40, 300, 50, ((size_t)1 << 26) + 1, 3, 132, 50, 0, {ok}});
    c.push_back({"plane_pitch_over", SRC, MASK, (uintptr_t)1 << 40, 300, 50, ((size_t)1 << 26) + 1, 3, 132, 50, P, {ok}});
    c.push_back({"src_pitch_over", SRC, MASK, (uintptr_t)1 << 40, ((size_t)1 << 26) + 1, 3, 320, 60, 132, 50, 0, {ok}});
    c.push_back({"dst_rows_over", SRC, MASK, (uintptr_t)1 << 40, 300, 50, 320, 60, 4, (size_t)1 << 31, 0, {{0, 0, 4, 3, 0, 0, 0, 0, 255, 0}}});
    c.push_back({"src_rows_over", (uintptr_t)1 << 44, MASK, DST, 4, (size_t)1 << 31, 320, 60, 132, 50, 0, {{0, 0, 4, 3, 0, 0, 0, 0, 255, 0}}});
    c.push_back({"mask_rows_over", SRC, (uintptr_t)1 << 44, DST, 300, 50, 4, (size_t)1 << 31, 132, 50, P, {{0, 0, 4, 3, 0, 0, 0, 0, 255, 0}}});
    c.push_back({"tall_image_last_rows", SRC, MASK, (uintptr_t)1 << 44, 300, 50, 320, 60, 4, 0x7fffffffu, 0, {{0, 0, 4, 50, 0, 0x7fffffff - 20, 7, 9, 77, 1}}});
    c.push_back({"too_many_tiles", 0, (uintptr_t)1 << 50, (uintptr_t)1 << 40, 0, 0, (size_t)1 << 26, (size_t)1 << 11, (size_t)1 << 26, (size_t)1 << 11, P | E,
                 {{0, 0, 1u << 26, 1u << 11, 0, 0, 0, 0, 255, 0}}});
    return c;
}

// the properties the kernel relies on, for small images: a count per destination pixel
void check_tables(const Case &cs, const fr::MaskTables &t)
{
    if (cs.ds * cs.dr > ((size_t)1 << 20)) return;
    const bool plane = cs.flags & FR_MASK_PLANE, erase = cs.flags & FR_MASK_ERASE;
    std::vector<uint8_t> want(cs.ds * cs.dr, 0), got(cs.ds * cs.dr, 0);
    for (size_t b = 0; b < t.clips.size(); ++b) {
        const fr::LayerClip &c = t.clips[b];
        if (cs.blits[b].opacity == 0) continue;
        for (uint32_t y = c.y0; y < c.y1; ++y)
            for (uint32_t x = c.x0; x < c.x1; ++x) want[(size_t)y * cs.ds + x]++;
    }
    for (const fr::MaskTile &tl : t.tiles) {
        require(tl.x % fr::LAYER_LANE_PX == 0, cs.name, "a tile's x is no multiple of the lane's pixels");
        require(tl.invert <= 1 && (tl.ov & 0xffu) != 0, cs.name, "a tile's invert or opacity");
        for (uint32_t y = tl.y; y < tl.y + fr::LAYER_TILE_H && y < tl.y1; ++y)
            for (uint32_t x = tl.x; x < tl.x + fr::LAYER_TILE_W; ++x) {
                if (x < tl.x0 || x >= tl.x1) continue;
                require(y < cs.dr && x < cs.ds, cs.name, "a tile pixel outside the destination");
                if (y < cs.dr && x < cs.ds) got[(size_t)y * cs.ds + x]++;
                const int64_t sx = (int64_t)tl.sx + (x - tl.x), sy = (int64_t)tl.sy + (y - tl.y);
                if (!erase) require(sx >= 0 && (uint64_t)sx < cs.ss && (uint64_t)sy < cs.sr, cs.name, "a tile pixel reads outside the layer");
                const int64_t mx = (int64_t)tl.mx + (x - tl.x), my = (int64_t)tl.my + (y - tl.y);
                require(mx >= 0 && (uint64_t)mx < cs.ms && (uint64_t)my < cs.mr, cs.name, "a tile pixel reads outside the mask");
            }
        if (tl.ov & fr::LAYER_DST_VEC)
            require((cs.dst + 4 * ((uint64_t)tl.y * cs.ds + tl.x)) % 16 == 0 && cs.ds % 4 == 0, cs.name, "LAYER_DST_VEC on unaligned rows");
        if (tl.ov & fr::LAYER_SRC_VEC)
            require(!erase && (cs.src + 4 * ((int64_t)tl.sy * (int64_t)cs.ss + tl.sx)) % 16 == 0 && cs.ss % 4 == 0, cs.name, "LAYER_SRC_VEC on unaligned rows");
        if (tl.ov & fr::LAYER_MASK_VEC) {
            const int64_t at = (int64_t)cs.mask + (plane ? 1 : 4) * ((int64_t)tl.my * (int64_t)cs.ms + tl.mx);
            require(at % (plane ? 4 : 16) == 0 && cs.ms % 4 == 0, cs.name, "LAYER_MASK_VEC on unaligned rows");
        }
    }
    require(want == got, cs.name, "the tiles do not cover every pixel of the clipped rectangles exactly once");
    for (uint8_t v : want) require(v <= 1, cs.name, "clipped rectangles overlap");
}

}  // namespace

int main()
{
    for (const Case &cs : cases()) {
        const fr::MaskIn in{cs.src, cs.mask, cs.dst, cs.ss, cs.sr, cs.ms, cs.mr, cs.ds, cs.dr, cs.null_blits ? nullptr : cs.blits.data(), (uint32_t)cs.blits.size(), cs.flags};
        fr::MaskTables t;
        clear_error();
        const int rc = fr::layer_mask_tables(in, t);
        std::vector<std::string> bl, cl, og, tl;
        for (const fr_layer_mask_blit &b : cs.blits)
            bl.push_back(fmt("%u,%u,%u,%u,%d,%d,%u,%u,%u,%u", b.src_x, b.src_y, b.w, b.h, b.dst_x, b.dst_y, b.mask_x, b.mask_y, b.opacity, b.invert));
        printf("%s rc=%d in=%llu,%llu,%llu,%zu,%zu,%zu,%zu,%zu,%zu,%u blits=%s%s | ", cs.name.c_str(), rc, (unsigned long long)cs.src, (unsigned long long)cs.mask,
               (unsigned long long)cs.dst, cs.ss, cs.sr, cs.ms, cs.mr, cs.ds, cs.dr, cs.flags, join(bl).c_str(), cs.null_blits ? " null" : "");
        if (rc) {
            printf("err=%s\n", last_error());
            continue;
        }
        for (const fr::LayerClip &c : t.clips) cl.push_back(fmt("%u,%u,%u,%u,%u,%u", c.x0, c.y0, c.x1, c.y1, c.sx, c.sy));
        for (const fr::MaskOrigin &g : t.origins) og.push_back(fmt("%u,%u", g.mx, g.my));
        for (const fr::MaskTile &x : t.tiles)
            tl.push_back(fmt("%u,%u,%u,%u,%u,%d,%u,%u,%d,%u,%u", x.x, x.y, x.x0, x.x1, x.y1, x.sx, x.sy, x.ov, x.mx, x.my, x.invert));
        printf("pixels=%llu clips=%s origins=%s tiles=%s\n", (unsigned long long)t.pixels, join(cl).c_str(), join(og).c_str(), join(tl).c_str());
        check_tables(cs, t);
    }
    return exit_status();
}

// layer_lcd_selftest.cpp — the host side of fr_layer_lcd (csrc/fr_layer_lcd_plan.cpp) on the CPU: links
// fr_layer_lcd_plan.o and nothing else of the library.  No GPU; the device pointers are made-up integers.  It prints one
// line per case,
//   <case> rc=<code> in=<cov>,<dst>,<cov stride>,<cov rows>,<dst stride>,<dst rows>,<flags> weights=<five values | default>
//          blits=<sx,sy,w,h,dx,dy,r,g,b,a;...> | w=<five values> clips=<x0,y0,x1,y1,sx,sy;...>
//          tiles=<x,y,x0,x1,y1,sy,sq,q0,q1,rgba,vec;...>
// with the word null behind the blits for a NULL table and "| err=<the message left>" for a refused call.
// tests/test_layer_lcd_tables.py restates the checks, the clipping and the tiling in Python from the inputs of each line
// and compares.  After each line it checks what the kernel relies on (every pixel of a clipped rectangle in exactly one
// tile; every sub-pixel of a tile pixel inside the window and the window inside the plane; the vector flags only where
// the addresses are aligned) and fails with the case and the property on stderr.
#include "../csrc/fr_layer_lcd_plan.hpp"
#include "selftest.hpp"

#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

using namespace selftest;

namespace {

struct Case {
    std::string name;
    uintptr_t cov, dst;
    size_t cs, cr, ds, dr;
    uint32_t flags;
    std::vector<fr_lcd_blit> blits;
    std::vector<uint16_t> weights = {};        // empty: NULL, the default filter
    bool null_blits = false;
};

constexpr uintptr_t COV = 0x10000000u, DST = 0x20000000u;
constexpr size_t P26 = (size_t)1 << 26;

fr_lcd_blit B(uint32_t sx, uint32_t sy, uint32_t w, uint32_t h, int32_t dx, int32_t dy, uint8_t r = 255, uint8_t g = 255, uint8_t b = 255, uint8_t a = 255)
{
    return fr_lcd_blit{sx, sy, w, h, dx, dy, {r, g, b, a}};
}

// the plane is 900 x 50 (300 pixels wide) unless a case says otherwise; the image 130 x 50 in rows of 131 or 132
std::vector<Case> cases()
{
    std::vector<Case> c;
    c.push_back({"whole_plane_aligned", COV, DST, 384, 40, 128, 40, 0, {B(0, 0, 128, 40, 0, 0)}});
    c.push_back({"srgb_and_bgr", COV, DST, 384, 40, 128, 40, FR_LAYER_SRGB | FR_LCD_BGR, {B(0, 0, 128, 40, 0, 0, 9, 8, 7, 200)}});
    c.push_back({"negative_offsets", COV, DST, 900, 50, 131, 50, 0, {B(0, 0, 97, 41, -5, -7)}});
    c.push_back({"negative_offsets_aligned_rows", COV, DST, 900, 50, 132, 50, 0, {B(0, 0, 97, 41, -5, -7)}});
    c.push_back({"partly_outside_right_bottom", COV, DST, 900, 50, 132, 50, 0, {B(3, 2, 97, 41, 100, 30)}});
    c.push_back({"wholly_outside_right", COV, DST, 900, 50, 132, 50, 0, {B(0, 0, 10, 10, 132, 0)}});
    c.push_back({"wholly_outside_above", COV, DST, 900, 50, 132, 50, 0, {B(0, 0, 10, 10, 5, -10)}});
    c.push_back({"wholly_outside_left_by_min", COV, DST, 900, 50, 132, 50, 0, {B(0, 0, 10, 10, INT32_MIN, INT32_MIN)}});
    c.push_back({"far_right_max", COV, DST, 900, 50, 132, 50, 0, {B(0, 0, 10, 10, INT32_MAX, INT32_MAX)}});
    for (uint32_t w : {1u, 3u, 64u, 257u}) {
        c.push_back({"width_" + std::to_string(w), COV, DST, 900, 50, 512, 50, 0, {B(0, 0, w, 5, 8, 1)}});
        c.push_back({"width_" + std::to_string(w) + "_at_x3", COV, DST, 900, 50, 512, 50, 0, {B(1, 0, w, 17, 3, 1)}});
    }
    for (uint32_t sx : {0u, 1u, 2u, 3u})
        for (size_t pitch : {900u, 901u, 902u, 903u})
            c.push_back({"src_x_" + std::to_string(sx) + "_pitch_" + std::to_string(pitch), COV, DST, pitch, 50, 132, 50, 0, {B(sx, 0, 40, 10, 8, 0)}});
    for (uintptr_t off : {1u, 2u, 3u}) c.push_back({"cov_off_" + std::to_string(off), COV + off, DST, 900, 50, 132, 50, 0, {B(4 - (uint32_t)off, 0, 40, 10, 8, 0)}});
    c.push_back({"two_touching", COV, DST, 900, 50, 132, 50, 0, {B(0, 0, 20, 10, 10, 10), B(60, 0, 20, 10, 30, 10, 1, 2, 3, 4), B(0, 10, 40, 5, 10, 20)}});
    c.push_back({"two_overlap_by_one_pixel", COV, DST, 900, 50, 132, 50, 0, {B(0, 0, 20, 10, 10, 10), B(60, 0, 20, 10, 29, 19)}});
    c.push_back({"overlap_only_before_clipping", COV, DST, 900, 50, 132, 50, 0, {B(0, 0, 20, 10, -30, 0), B(0, 0, 20, 10, -25, 5)}});
    c.push_back({"window_last_element_in", COV, DST, 900, 50, 132, 50, 0, {B(609, 9, 97, 41, 0, 0)}});
    c.push_back({"window_one_element_out_right", COV, DST, 900, 50, 132, 50, 0, {B(610, 0, 97, 41, 0, 0)}});
    c.push_back({"window_one_row_out_below", COV, DST, 900, 50, 132, 50, 0, {B(0, 10, 97, 41, 0, 0)}});
    c.push_back({"window_wraps_uint32", COV, DST, 900, 50, 132, 50, 0, {B(UINT32_MAX, 0, 2, 2, 0, 0)}});
    c.push_back({"window_width_wraps_uint32", COV, DST, 900, 50, 132, 50, 0, {B(0, 0, 0x55555556u, 2, 0, 0)}});
    c.push_back({"zero_width_anywhere", COV, DST, 900, 50, 132, 50, 0, {B(5000, 5000, 0, 7, 0, 0), B(0, 0, 7, 0, 0, 0)}});
    c.push_back({"no_blits", COV, DST, 900, 50, 132, 50, 0, {}});
    c.push_back({"no_blits_null", COV, DST, 900, 50, 132, 50, 0, {}, {}, true});
    c.push_back({"weights_identity", COV, DST, 900, 50, 132, 50, 0, {B(0, 0, 10, 10, 0, 0)}, {0, 0, 256, 0, 0}});
    c.push_back({"weights_one_sided", COV, DST, 900, 50, 132, 50, 0, {B(0, 0, 10, 10, 0, 0)}, {256, 0, 0, 0, 0}});
    c.push_back({"weights_asymmetric", COV, DST, 900, 50, 132, 50, 0, {B(0, 0, 10, 10, 0, 0)}, {0, 16, 64, 176, 0}});
    c.push_back({"adjacent_images", COV, COV + 900 * 50, 900, 50, 132, 50, 0, {B(0, 0, 10, 10, 0, 0)}});
    c.push_back({"dst_4_aligned_only", COV, DST + 4, 900, 50, 132, 50, 0, {B(0, 0, 40, 10, 0, 0)}});
    c.push_back({"pitch_max", COV, (uintptr_t)1 << 40, P26, 3, P26, 3, 0, {B(P26 - 300, 0, 100, 3, P26 - 100, 0)}});
    c.push_back({"tall_image_last_rows", COV, (uintptr_t)1 << 44, 12, 50, 4, 0x7fffffffu, 0, {B(0, 0, 4, 50, 0, 0x7fffffff - 20, 1, 2, 3, 77)}});
    // every refusal, in the header's order
    c.push_back({"unknown_flag_4", COV, DST, 900, 50, 132, 50, 4, {B(0, 0, 10, 10, 0, 0)}});
    c.push_back({"text_flag_bits", COV, DST, 900, 50, 132, 50, FR_TEXT_SRGB | FR_TEXT_OVER, {B(0, 0, 10, 10, 0, 0)}});
    c.push_back({"cov_null", 0, DST, 900, 50, 132, 50, 0, {B(0, 0, 10, 10, 0, 0)}});
    c.push_back({"cov_pitch_over", COV, (uintptr_t)1 << 40, P26 + 1, 3, 132, 50, 0, {B(0, 0, 10, 3, 0, 0)}});
    c.push_back({"dst_null", COV, 0, 900, 50, 132, 50, 0, {B(0, 0, 10, 10, 0, 0)}});
    c.push_back({"dst_not_4_aligned", COV, DST + 1, 900, 50, 132, 50, 0, {B(0, 0, 10, 10, 0, 0)}});
    c.push_back({"dst_pitch_over", COV, (uintptr_t)1 << 40, 900, 50, P26 + 1, 3, 0, {B(0, 0, 10, 3, 0, 0)}});
    c.push_back({"dst_rows_over", COV, (uintptr_t)1 << 40, 900, 50, 4, (size_t)1 << 31, 0, {B(0, 0, 4, 3, 0, 0)}});
    c.push_back({"cov_rows_over", (uintptr_t)1 << 44, DST, 12, (size_t)1 << 31, 132, 50, 0, {B(0, 0, 4, 3, 0, 0)}});
    c.push_back({"blits_null", COV, DST, 900, 50, 132, 50, 0, {B(0, 0, 10, 10, 0, 0)}, {}, true});
    c.push_back({"weights_sum_255", COV, DST, 900, 50, 132, 50, 0, {B(0, 0, 10, 10, 0, 0)}, {8, 77, 85, 77, 8}});
    c.push_back({"weights_sum_257", COV, DST, 900, 50, 132, 50, 0, {B(0, 0, 10, 10, 0, 0)}, {8, 77, 87, 77, 8}});
    c.push_back({"weights_sum_wraps_uint16", COV, DST, 900, 50, 132, 50, 0, {B(0, 0, 10, 10, 0, 0)}, {65535, 257, 0, 0, 0}});
    c.push_back({"weights_refused_without_blits", COV, DST, 900, 50, 132, 50, 0, {}, {0, 0, 0, 0, 0}});
    c.push_back({"aliasing_same_memory", COV, COV, 900, 50, 132, 50, 0, {B(0, 0, 10, 10, 20, 0)}});
    c.push_back({"aliasing_last_byte", COV, COV + 900 * 50 - 4, 900, 50, 132, 50, 0, {B(0, 0, 10, 10, 0, 0)}});
    c.push_back({"aliasing_image_first", COV + 4 * 132 * 50 - 1, COV, 900, 50, 132, 50, 0, {B(0, 0, 10, 10, 0, 0)}});
    c.push_back({"tiles_over", COV, (uintptr_t)1 << 44, (size_t)3 << 16, ((size_t)1 << 18) + 1, (size_t)1 << 16, ((size_t)1 << 18) + 1, 0, {B(0, 0, 1 << 16, (1 << 18) + 1, 0, 0)}});
    c.push_back({"tiles_over_by_the_lead", COV, (uintptr_t)1 << 44, (size_t)3 << 16, (size_t)1 << 18, ((size_t)1 << 16) + 4, (size_t)1 << 18, 0, {B(0, 0, 1 << 16, 1 << 18, 1, 0)}});
    // the validation order, one case per rule: the earlier rule's code wins
    c.push_back({"order_flag_before_cov", 0, DST, 900, 50, 132, 50, 4, {B(0, 0, 10, 10, 0, 0)}});
    c.push_back({"order_cov_before_dst", COV, DST + 2, P26 + 1, 50, 132, 50, 0, {B(0, 0, 10, 10, 0, 0)}});
    c.push_back({"order_dst_before_rows", COV, DST + 2, 900, 50, 4, (size_t)1 << 31, 0, {B(0, 0, 4, 3, 0, 0)}});
    c.push_back({"order_rows_before_null_blits", COV, (uintptr_t)1 << 40, 900, 50, 4, (size_t)1 << 31, 0, {B(0, 0, 4, 3, 0, 0)}, {}, true});
    c.push_back({"order_null_blits_before_weights", COV, DST, 900, 50, 132, 50, 0, {B(0, 0, 10, 10, 0, 0)}, {1, 0, 0, 0, 0}, true});
    c.push_back({"order_weights_before_window", COV, DST, 900, 50, 132, 50, 0, {B(895, 0, 10, 10, 0, 0)}, {1, 0, 0, 0, 0}});
    c.push_back({"order_window_before_overlap", COV, DST, 900, 50, 132, 50, 0, {B(0, 0, 20, 10, 10, 10), B(0, 0, 20, 10, 10, 10), B(895, 0, 10, 10, 0, 0)}});
    c.push_back({"order_overlap_before_aliasing", COV, COV, 900, 50, 132, 50, 0, {B(0, 0, 20, 10, 10, 10), B(0, 0, 20, 10, 10, 10)}});
    c.push_back({"order_aliasing_before_tiles", (uintptr_t)1 << 44, (uintptr_t)1 << 44, (size_t)3 << 16, ((size_t)1 << 18) + 1, (size_t)1 << 16, ((size_t)1 << 18) + 1, 0,
                 {B(0, 0, 1 << 16, (1 << 18) + 1, 0, 0)}});
    return c;
}

// the properties the kernel relies on; the per-pixel count only for small images
void check_tables(const Case &cs, const fr::LcdTables &t)
{
    const bool small = cs.ds * cs.dr <= ((size_t)1 << 20);
    std::vector<uint8_t> want(small ? cs.ds * cs.dr : 0, 0), got(want.size(), 0);
    if (small)
        for (const fr::LayerClip &c : t.clips)
            for (uint32_t y = c.y0; y < c.y1; ++y)
                for (uint32_t x = c.x0; x < c.x1; ++x) want[(size_t)y * cs.ds + x]++;
    for (const fr::LcdTile &tl : t.tiles) {
        require(tl.x % fr::LAYER_LANE_PX == 0 && tl.x + fr::LAYER_LANE_PX > tl.x0, cs.name, "a tile's x is no multiple of the lane's pixels, or a whole group left of the blit");
        require(tl.x1 <= cs.ds && tl.y1 <= cs.dr && tl.y < tl.y1 && tl.x < tl.x1, cs.name, "a tile outside the destination");
        require(tl.q0 <= tl.q1 && tl.q1 <= cs.cs && (tl.q1 - tl.q0) % 3 == 0, cs.name, "the window leaves the plane's row");
        const uint32_t rows = std::min(tl.y + fr::LAYER_TILE_H, tl.y1) - tl.y;
        require((uint64_t)tl.sy + rows <= cs.cr, cs.name, "a tile row below the plane");
        const uint32_t xa = std::max(tl.x, tl.x0), xb = std::min(tl.x + fr::LAYER_TILE_W, tl.x1);
        // sub-pixel 0 of the tile's first pixel and sub-pixel 2 of its last lie in the window
        require((int64_t)tl.sq + 3 * (int64_t)(xa - tl.x) >= tl.q0 && (int64_t)tl.sq + 3 * (int64_t)(xb - tl.x) <= tl.q1, cs.name, "a tile pixel's sub-pixels leave the window");
        require(tl.sq >= -9, cs.name, "sq more than three pixels below element 0");
        if (small)
            for (uint32_t y = tl.y; y < tl.y + rows; ++y)
                for (uint32_t x = xa; x < xb; ++x) got[(size_t)y * cs.ds + x]++;
        if (tl.vec & fr::LAYER_DST_VEC)
            require((cs.dst + 4 * ((uint64_t)tl.y * cs.ds + tl.x)) % 16 == 0 && cs.ds % 4 == 0, cs.name, "LAYER_DST_VEC on unaligned rows");
        if (tl.vec & fr::LAYER_SRC_VEC)
            require(((int64_t)cs.cov + (int64_t)tl.sy * (int64_t)cs.cs + tl.sq) % 4 == 0 && cs.cs % 4 == 0, cs.name, "LAYER_SRC_VEC on unaligned elements");
    }
    require(want == got, cs.name, "the tiles do not cover every pixel of the clipped rectangles exactly once");
    for (uint8_t v : want) require(v <= 1, cs.name, "clipped rectangles overlap");
}

}  // namespace

int main()
{
    for (const Case &cs : cases()) {
        const fr::LcdIn in{cs.cov, cs.dst, cs.cs, cs.cr, cs.ds, cs.dr, cs.null_blits ? nullptr : cs.blits.data(), (uint32_t)cs.blits.size(),
                           cs.weights.empty() ? nullptr : cs.weights.data(), cs.flags};
        fr::LcdTables t;
        clear_error();
        const int rc = fr::layer_lcd_tables(in, t);
        std::vector<std::string> bl, cl, tl;
        for (const fr_lcd_blit &b : cs.blits)
            bl.push_back(fmt("%u,%u,%u,%u,%d,%d,%u,%u,%u,%u", b.src_x, b.src_y, b.w, b.h, b.dst_x, b.dst_y, b.rgba[0], b.rgba[1], b.rgba[2], b.rgba[3]));
        const std::string ws = cs.weights.empty() ? "default" : fmt("%u,%u,%u,%u,%u", cs.weights[0], cs.weights[1], cs.weights[2], cs.weights[3], cs.weights[4]);
        printf("%s rc=%d in=%llu,%llu,%zu,%zu,%zu,%zu,%u weights=%s blits=%s%s | ", cs.name.c_str(), rc, (unsigned long long)cs.cov, (unsigned long long)cs.dst, cs.cs, cs.cr,
               cs.ds, cs.dr, cs.flags, ws.c_str(), join(bl).c_str(), cs.null_blits ? " null" : "");
        if (rc) {
            printf("err=%s\n", last_error());
            continue;
        }
        for (const fr::LayerClip &c : t.clips) cl.push_back(fmt("%u,%u,%u,%u,%u,%u", c.x0, c.y0, c.x1, c.y1, c.sx, c.sy));
        for (const fr::LcdTile &x : t.tiles) tl.push_back(fmt("%u,%u,%u,%u,%u,%u,%d,%u,%u,%u,%u", x.x, x.y, x.x0, x.x1, x.y1, x.sy, x.sq, x.q0, x.q1, x.rgba, x.vec));
        printf("w=%u,%u,%u,%u,%u clips=%s tiles=%s\n", t.w[0], t.w[1], t.w[2], t.w[3], t.w[4], join(cl).c_str(), join(tl).c_str());
        check_tables(cs, t);
    }
    return exit_status();
}

// layer_selftest.cpp — the host side of fr_layer_over and fr_layer_unpremultiply (csrc/fr_layer_plan.cpp) on the CPU: links
// fr_layer_plan.o and nothing else of the library.  No GPU; the device pointers are made-up integers.  It prints one line
// per case,
//   <case> rc=<code> in=<src>,<dst>,<src stride>,<src rows>,<dst stride>,<dst rows>,<flags> blits=<sx,sy,w,h,dx,dy,o;...> |
//          opacity=<0|1> pixels=<n> clips=<x0,y0,x1,y1,sx,sy;...> tiles=<x,y,x0,x1,y1,sx,sy,ov;...>
// or, for a refused call, "| err=<the message left>" behind the bar.  tests/test_layer_tables.py restates the clipping and
// the tiling in Python from the inputs of each line and compares.  After the lines it checks the tables' own properties
// (every pixel of a clipped rectangle in exactly one tile, no tile pixel outside it, the vector flags only where the
// addresses are 16-byte aligned) and fails with the case and the property on stderr.
#include "../csrc/fr_layer_plan.hpp"
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
    std::vector<fr_layer_blit> blits;
    bool null_blits = false;
};

constexpr uintptr_t SRC = 0x10000000u, DST = 0x20000000u;

// the layer is 300 x 50 (stride 300) unless a case says otherwise; the image 130 x 50 in rows of 131 or 132
std::vector<Case> cases()
{
    std::vector<Case> c;
    c.push_back({"whole_layer_aligned", SRC, DST, 128, 40, 132, 50, 0, {{0, 0, 128, 40, 0, 0, 255}}});
    c.push_back({"negative_offsets", SRC, DST, 300, 50, 131, 50, 0, {{0, 0, 97, 41, -5, -7, 255}}});
    c.push_back({"negative_offsets_aligned_rows", SRC, DST, 300, 50, 132, 50, 0, {{0, 0, 97, 41, -5, -7, 255}}});
    c.push_back({"partly_outside_right_bottom", SRC, DST, 300, 50, 132, 50, 0, {{3, 2, 97, 41, 100, 30, 255}}});
    c.push_back({"wholly_outside_right", SRC, DST, 300, 50, 132, 50, 0, {{0, 0, 10, 10, 132, 0, 255}}});
    c.push_back({"wholly_outside_above", SRC, DST, 300, 50, 132, 50, 0, {{0, 0, 10, 10, 5, -10, 255}}});
    c.push_back({"wholly_outside_left_by_min", SRC, DST, 300, 50, 132, 50, 0, {{0, 0, 10, 10, INT32_MIN, INT32_MIN, 255}}});
    c.push_back({"far_right_max", SRC, DST, 300, 50, 132, 50, 0, {{0, 0, 10, 10, INT32_MAX, INT32_MAX, 255}}});
    for (uint32_t w : {1u, 3u, 63u, 64u, 65u, 257u}) {
        c.push_back({"width_" + std::to_string(w), SRC, DST, 300, 50, 512, 50, 0, {{0, 0, w, 5, 8, 1, 255}}});
        c.push_back({"width_" + std::to_string(w) + "_at_x3", SRC, DST, 300, 50, 512, 50, 0, {{1, 0, w, 17, 3, 1, 255}}});
    }
    c.push_back({"two_touching", SRC, DST, 300, 50, 132, 50, 0, {{0, 0, 20, 10, 10, 10, 255}, {20, 0, 20, 10, 30, 10, 255}, {0, 10, 40, 5, 10, 20, 255}}});
    c.push_back({"two_overlap_by_one_pixel", SRC, DST, 300, 50, 132, 50, 0, {{0, 0, 20, 10, 10, 10, 255}, {20, 0, 20, 10, 29, 19, 255}}});
    c.push_back({"overlap_only_before_clipping", SRC, DST, 300, 50, 132, 50, 0, {{0, 0, 20, 10, -30, 0, 255}, {0, 0, 20, 10, -25, 5, 255}}});
    c.push_back({"overlap_with_an_opacity_0_blit", SRC, DST, 300, 50, 132, 50, 0, {{0, 0, 20, 10, 10, 10, 0}, {20, 0, 20, 10, 29, 19, 255}}});
    c.push_back({"source_one_pixel_out_right", SRC, DST, 300, 50, 132, 50, 0, {{204, 0, 97, 41, 0, 0, 255}}});
    c.push_back({"source_last_column_in", SRC, DST, 300, 50, 132, 50, 0, {{203, 9, 97, 41, 0, 0, 255}}});
    c.push_back({"source_one_pixel_out_below", SRC, DST, 300, 50, 132, 50, 0, {{0, 10, 97, 41, 0, 0, 255}}});
    c.push_back({"opacity_256", SRC, DST, 300, 50, 132, 50, 0, {{0, 0, 10, 10, 0, 0, 256}}});
    c.push_back({"opacity_255_and_128", SRC, DST, 300, 50, 132, 50, FR_LAYER_SRGB, {{0, 0, 10, 10, 0, 0, 255}, {0, 0, 10, 10, 20, 0, 128}}});
    c.push_back({"opacity_0_has_no_tile", SRC, DST, 300, 50, 132, 50, 0, {{0, 0, 10, 10, 0, 0, 0}, {0, 0, 10, 10, 20, 0, 255}}});
    c.push_back({"zero_width_anywhere", SRC, DST, 300, 50, 132, 50, 0, {{1000, 1000, 0, 7, 0, 0, 255}, {0, 0, 7, 0, 0, 0, 255}}});
    c.push_back({"aliasing_same_image", SRC, SRC, 300, 50, 300, 50, 0, {{0, 0, 10, 10, 20, 0, 255}}});
    c.push_back({"aliasing_last_byte", SRC, SRC + 4 * 300 * 50 - 4, 300, 50, 132, 50, 0, {{0, 0, 10, 10, 0, 0, 255}}});
    c.push_back({"adjacent_images", SRC, SRC + 4 * 300 * 50, 300, 50, 132, 50, 0, {{0, 0, 10, 10, 0, 0, 255}}});
    c.push_back({"src_not_4_aligned", SRC + 2, DST, 300, 50, 132, 50, 0, {{0, 0, 10, 10, 0, 0, 255}}});
    c.push_back({"dst_not_4_aligned", SRC, DST + 1, 300, 50, 132, 50, 0, {{0, 0, 10, 10, 0, 0, 255}}});
    c.push_back({"dst_4_aligned_only", SRC, DST + 4, 300, 50, 132, 50, 0, {{0, 0, 40, 10, 0, 0, 255}}});
    c.push_back({"src_4_aligned_only", SRC + 8, DST, 300, 50, 132, 50, 0, {{0, 0, 40, 10, 0, 0, 255}}});
    c.push_back({"src_x_unaligned", SRC, DST, 300, 50, 132, 50, 0, {{5, 0, 40, 10, 8, 0, 255}}});
    c.push_back({"src_x_matches_dst_x_mod_4", SRC, DST, 300, 50, 132, 50, 0, {{6, 0, 40, 10, 10, 0, 255}}});
    c.push_back({"src_null", 0, DST, 300, 50, 132, 50, 0, {{0, 0, 10, 10, 0, 0, 255}}});
    c.push_back({"dst_null", SRC, 0, 300, 50, 132, 50, 0, {{0, 0, 10, 10, 0, 0, 255}}});
    c.push_back({"blits_null", SRC, DST, 300, 50, 132, 50, 0, {{0, 0, 10, 10, 0, 0, 255}}, true});
    c.push_back({"no_blits", SRC, DST, 300, 50, 132, 50, 0, {}});
    c.push_back({"unknown_flag_2", SRC, DST, 300, 50, 132, 50, 2, {{0, 0, 10, 10, 0, 0, 255}}});
    c.push_back({"text_flag_bits", SRC, DST, 300, 50, 132, 50, FR_TEXT_SRGB | FR_TEXT_OVER, {{0, 0, 10, 10, 0, 0, 255}}});
    c.push_back({"pitch_max", SRC, (uintptr_t)1 << 40, 300, 50, (size_t)1 << 26, 3, 0, {{0, 0, 300, 3, (1 << 26) - 100, 0, 255}}});
    c.push_back({"pitch_over", SRC, (uintptr_t)1 << 40, 300, 50, ((size_t)1 << 26) + 1, 3, 0, {{0, 0, 10, 3, 0, 0, 255}}});
    c.push_back({"rows_over", SRC, (uintptr_t)1 << 40, 300, 50, 4, (size_t)1 << 31, 0, {{0, 0, 4, 3, 0, 0, 255}}});
    c.push_back({"tall_image_last_rows", SRC, (uintptr_t)1 << 44, 300, 50, 4, 0x7fffffffu, 0, {{0, 0, 4, 50, 0, 0x7fffffff - 20, 77}}});
    return c;
}

// the properties the kernel relies on, for small images: a count per destination pixel
void check_tables(const Case &cs, const fr::LayerTables &t)
{
    if (cs.ds * cs.dr > ((size_t)1 << 20)) return;
    std::vector<uint8_t> want(cs.ds * cs.dr, 0), got(cs.ds * cs.dr, 0);
    for (size_t b = 0; b < t.clips.size(); ++b) {
        const fr::LayerClip &c = t.clips[b];
        if (cs.blits[b].opacity == 0) continue;
        for (uint32_t y = c.y0; y < c.y1; ++y)
            for (uint32_t x = c.x0; x < c.x1; ++x) want[(size_t)y * cs.ds + x]++;
    }
    for (const fr::LayerTile &tl : t.tiles) {
        require(tl.x % fr::LAYER_LANE_PX == 0, cs.name, "a tile's x is no multiple of the lane's pixels");
        for (uint32_t y = tl.y; y < tl.y + fr::LAYER_TILE_H && y < tl.y1; ++y)
            for (uint32_t x = tl.x; x < tl.x + fr::LAYER_TILE_W; ++x) {
                if (x < tl.x0 || x >= tl.x1) continue;
                require(y < cs.dr && x < cs.ds, cs.name, "a tile pixel outside the destination");
                if (y < cs.dr && x < cs.ds) got[(size_t)y * cs.ds + x]++;
                const int64_t sx = (int64_t)tl.sx + (x - tl.x), sy = (int64_t)tl.sy + (y - tl.y);
                require(sx >= 0 && (uint64_t)sx < cs.ss && (uint64_t)sy < cs.sr, cs.name, "a tile pixel reads outside the layer");
            }
        if (tl.ov & fr::LAYER_DST_VEC)
            require((cs.dst + 4 * ((uint64_t)tl.y * cs.ds + tl.x)) % 16 == 0 && cs.ds % 4 == 0, cs.name, "LAYER_DST_VEC on unaligned rows");
        if (tl.ov & fr::LAYER_SRC_VEC)
            require((cs.src + 4 * ((int64_t)tl.sy * (int64_t)cs.ss + tl.sx)) % 16 == 0 && cs.ss % 4 == 0, cs.name, "LAYER_SRC_VEC on unaligned rows");
    }
    require(want == got, cs.name, "the tiles do not cover every pixel of the clipped rectangles exactly once");
    for (uint8_t v : want) require(v <= 1, cs.name, "clipped rectangles overlap");
}

}  // namespace

int main()
{
    for (const Case &cs : cases()) {
        const fr::LayerIn in{cs.src, cs.dst, cs.ss, cs.sr, cs.ds, cs.dr, cs.null_blits ? nullptr : cs.blits.data(), (uint32_t)cs.blits.size(), cs.flags};
        fr::LayerTables t;
        clear_error();
        const int rc = fr::layer_tables(in, t);
        std::vector<std::string> bl, cl, tl;
        for (const fr_layer_blit &b : cs.blits) bl.push_back(fmt("%u,%u,%u,%u,%d,%d,%u", b.src_x, b.src_y, b.w, b.h, b.dst_x, b.dst_y, b.opacity));
        printf("%s rc=%d in=%llu,%llu,%zu,%zu,%zu,%zu,%u blits=%s%s | ", cs.name.c_str(), rc, (unsigned long long)cs.src, (unsigned long long)cs.dst, cs.ss, cs.sr,
               cs.ds, cs.dr, cs.flags, join(bl).c_str(), cs.null_blits ? " null" : "");
        if (rc) {
            printf("err=%s\n", last_error());
            continue;
        }
        for (const fr::LayerClip &c : t.clips) cl.push_back(fmt("%u,%u,%u,%u,%u,%u", c.x0, c.y0, c.x1, c.y1, c.sx, c.sy));
        for (const fr::LayerTile &x : t.tiles) tl.push_back(fmt("%u,%u,%u,%u,%u,%d,%u,%u", x.x, x.y, x.x0, x.x1, x.y1, x.sx, x.sy, x.ov));
        printf("opacity=%d pixels=%llu clips=%s tiles=%s\n", t.opacity ? 1 : 0, (unsigned long long)t.pixels, join(cl).c_str(), join(tl).c_str());
        check_tables(cs, t);
    }
    // fr_layer_unpremultiply's window
    struct { const char *name; uintptr_t p; size_t stride; uint32_t w, h; } W[] = {
        {"window/inside", DST, 131, 100, 40}, {"window/whole_row", DST, 131, 131, 1}, {"window/wider_than_rows", DST, 131, 132, 1},
        {"window/null", 0, 131, 10, 10}, {"window/not_4_aligned", DST + 2, 131, 10, 10}, {"window/empty", DST, 131, 0, 10},
        {"window/pitch_over", DST, ((size_t)1 << 26) + 1, 10, 10}, {"window/too_many_tiles", DST, (size_t)1 << 26, 1u << 26, 1u << 10},
    };
    for (const auto &w : W) {
        clear_error();
        const int rc = fr::layer_window_check(w.p, w.stride, w.w, w.h);
        printf("%s rc=%d in=%llu,%zu,%u,%u | %s%s\n", w.name, rc, (unsigned long long)w.p, w.stride, w.w, w.h, rc ? "err=" : "ok", rc ? last_error() : "");
    }
    return exit_status();
}

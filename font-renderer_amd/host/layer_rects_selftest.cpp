// layer_rects_selftest.cpp — the host side of fr_layer_rects (csrc/fr_layer_rects_plan.cpp) on the CPU: links
// fr_layer_rects_plan.o and nothing else of the library.  No GPU; the device pointer is a made-up integer.  It prints one
// line per case,
//   <case> rc=<code> in=<dst>,<dst stride>,<dst rows>,<flags> rects=<x0,y0,x1,y1,r,g,b,a;...> |
//          vec=<0|1> recs=<x0,y0,x1,y1,rgba,index;...> tiles=<x,y,first,count;...> list=<record;...>
// or, for a refused call, "| err=<the message left>" behind the bar.  tests/test_layer_rects_tables.py restates the clipping
// and the binning in Python from the inputs of each line and compares.  After the lines it checks the tables' own
// properties (the tiles distinct, on the grid and in order; every list ascending; a record in a tile's list exactly when
// its bounding box meets the tile) and fails with the case and the property on stderr.
#include "../csrc/fr_layer_rects_plan.hpp"
#include "selftest.hpp"

#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

using namespace selftest;

namespace {

struct Case {
    std::string name;
    uintptr_t dst;
    size_t ds, dr;
    uint32_t flags;
    std::vector<fr_layer_rect> rects;
    bool null_rects = false;
};

constexpr uintptr_t DST = 0x20000000u;
constexpr int32_t MAXI = INT32_MAX, MINI = INT32_MIN;

fr_layer_rect R(int64_t x0, int64_t y0, int64_t x1, int64_t y1, uint8_t a = 255)
{
    return fr_layer_rect{(int32_t)x0, (int32_t)y0, (int32_t)x1, (int32_t)y1, {10, 20, 30, a}};
}

// the image is 130 x 50 in rows of 131 or 132 unless a case says otherwise
std::vector<Case> cases()
{
    std::vector<Case> c;
    c.push_back({"one_pixel_aligned", DST, 132, 50, 0, {R(64, 64, 128, 128)}});
    c.push_back({"sub_pixel", DST, 132, 50, 0, {R(70, 70, 71, 71)}});
    c.push_back({"whole_image", DST, 132, 50, 0, {R(0, 0, 132 * 64, 50 * 64)}});
    c.push_back({"rows131_no_vec", DST, 131, 50, 0, {R(0, 0, 131 * 64, 50 * 64)}});
    c.push_back({"dst_4_aligned_only", DST + 4, 132, 50, 0, {R(0, 0, 640, 640)}});
    c.push_back({"negative_edges", DST, 132, 50, 0, {R(-1000, -1000, 100, 100)}});
    c.push_back({"far_outside", DST, 132, 50, 0, {R(132 * 64, 0, 133 * 64, 64), R(0, 50 * 64, 64, 51 * 64), R(-200, -200, 0, 0), R(MAXI - 5, MAXI - 5, MAXI, MAXI)}});
    c.push_back({"extreme_edges", DST, 132, 50, 0, {R(MINI, MINI, MAXI, MAXI)}});
    c.push_back({"inverted", DST, 132, 50, 0, {R(640, 640, 64, 64), R(64, 640, 640, 64), R(MAXI, MAXI, MINI, MINI), R(64, 64, 64, 640)}});
    c.push_back({"transparent_dropped", DST, 132, 50, 0, {R(0, 0, 640, 640, 0), R(64, 64, 128, 128, 1), R(0, 0, 64, 64, 0)}});
    c.push_back({"all_transparent", DST, 132, 50, 0, {R(0, 0, 640, 640, 0)}});
    c.push_back({"no_rects", DST, 132, 50, 0, {}});
    c.push_back({"tile_row_border", DST, 132, 50, 0, {R(64, 15 * 64 + 63, 128, 16 * 64 + 1)}});
    c.push_back({"ends_on_tile_row_border", DST, 132, 50, 0, {R(64, 15 * 64, 128, 16 * 64)}});
    c.push_back({"tile_column_border", DST, 600, 20, 0, {R(255 * 64 + 63, 64, 256 * 64 + 1, 128), R(510 * 64, 0, 513 * 64, 17 * 64)}});
    c.push_back({"ends_on_tile_column_border", DST, 600, 20, 0, {R(200 * 64, 64, 256 * 64, 128)}});
    c.push_back({"overlapping_in_order", DST, 600, 40, FR_LAYER_SRGB, {R(300 * 64, 0, 400 * 64, 40 * 64), R(0, 0, 600 * 64, 64, 0), R(0, 10 * 64, 600 * 64, 20 * 64),
                                                                      R(250 * 64, 5 * 64, 260 * 64, 6 * 64), R(0, 0, 64, 64)}});
    {
        Case many{"many_in_one_tile", DST, 132, 50, 0, {}};
        for (int i = 0; i < 300; ++i) many.rects.push_back(R(64 + 13 * (i % 17), 64 + 7 * (i % 23), 64 + 13 * (i % 17) + 5 * i, 64 + 7 * (i % 23) + 3 * i, (uint8_t)(i % 4 ? 200 : 0)));
        c.push_back(many);
    }
    // too far apart for the counting sort over the tiles between them: the sorted pairs
    c.push_back({"far_apart_in_a_large_image", (uintptr_t)1 << 44, (size_t)1 << 26, 1 << 20, 0,
                 {R(MAXI - 200, (1 << 26) - 200, MAXI, 1 << 26), R(0, 0, 64, 64), R(32, 32, 20000, 1100, 7), R(MAXI - 100, (1 << 26) - 2000, MAXI, 1 << 26)}});
    c.push_back({"rects_null", DST, 132, 50, 0, {R(0, 0, 64, 64)}, true});
    c.push_back({"dst_null", 0, 132, 50, 0, {R(0, 0, 64, 64)}});
    c.push_back({"dst_not_4_aligned", DST + 2, 132, 50, 0, {R(0, 0, 64, 64)}});
    c.push_back({"unknown_flag_2", DST, 132, 50, 2, {R(0, 0, 64, 64)}});
    c.push_back({"text_flag_bits", DST, 132, 50, FR_TEXT_SRGB | FR_TEXT_OVER, {R(0, 0, 64, 64)}});
    c.push_back({"pitch_max", (uintptr_t)1 << 40, (size_t)1 << 26, 3, 0, {R(MAXI - 200, 0, MAXI, 3 * 64)}});
    c.push_back({"pitch_over", (uintptr_t)1 << 40, ((size_t)1 << 26) + 1, 3, 0, {R(0, 0, 64, 64)}});
    c.push_back({"rows_over", (uintptr_t)1 << 40, 4, (size_t)1 << 31, 0, {R(0, 0, 64, 64)}});
    c.push_back({"tall_image_last_reachable_rows", (uintptr_t)1 << 44, 4, 0x7fffffffu, 0, {R(0, MAXI - 200, 4 * 64, MAXI)}});
    // the validation order, one case per rule: the earlier rule's code wins
    c.push_back({"order_flag_before_dst", 0, 132, 50, 2, {R(0, 0, 64, 64)}});
    c.push_back({"order_dst_before_pitch", DST + 1, ((size_t)1 << 26) + 1, 50, 0, {R(0, 0, 64, 64)}});
    c.push_back({"order_pitch_before_rows", DST, ((size_t)1 << 26) + 1, (size_t)1 << 31, 0, {R(0, 0, 64, 64)}});
    c.push_back({"order_rows_before_null_rects", DST, 132, (size_t)1 << 31, 0, {R(0, 0, 64, 64)}, true});
    c.push_back({"order_null_rects_before_limits", (uintptr_t)1 << 44, (size_t)1 << 26, 1 << 20, 0, {R(0, 0, MAXI, MAXI)}, true});
    // the limits: 2^17 x 2^6 tiles in one rectangle; the same number in two rectangles (counted tile by tile); 5 x 2^22 pairs
    c.push_back({"tiles_over_one_rect", (uintptr_t)1 << 44, (size_t)1 << 26, 1 << 10, 0, {R(0, 0, MAXI, 1 << 16)}});
    c.push_back({"tiles_at_limit_pairs_over", (uintptr_t)1 << 44, (size_t)1 << 26, 1 << 10, 0,
                 {R(0, 0, MAXI, 1 << 15), R(0, 0, MAXI, 1 << 15), R(0, 0, MAXI, 1 << 15), R(0, 0, MAXI, 1 << 15), R(0, 0, MAXI, 1 << 15)}});
    c.push_back({"tiles_over_two_rects", (uintptr_t)1 << 44, (size_t)1 << 26, 1 << 10, 0, {R(0, 0, MAXI, 1 << 14), R(0, 1 << 14, MAXI, (1 << 15) + 1)}});
    return c;
}

// the properties the kernel relies on
void check_tables(const Case &cs, const fr::RectsTables &t)
{
    size_t next = 0, listed = 0;
    for (size_t k = 0; k < t.tiles.size(); ++k) {
        const fr::RectTile &tl = t.tiles[k];
        require(tl.x % fr::LAYER_TILE_W == 0 && tl.y % fr::LAYER_TILE_H == 0, cs.name, "a tile off the grid");
        require(tl.x < cs.ds && tl.y < cs.dr, cs.name, "a tile outside the image");
        if (k) require(tl.y > t.tiles[k - 1].y || (tl.y == t.tiles[k - 1].y && tl.x > t.tiles[k - 1].x), cs.name, "tiles out of order or listed twice");
        require(tl.first == next && tl.count > 0 && (size_t)tl.first + tl.count <= t.list.size(), cs.name, "a tile's range of the list");
        next = (size_t)tl.first + tl.count;
        for (uint32_t i = 0; i < tl.count && (size_t)tl.first + i < t.list.size(); ++i) {
            const uint32_t r = t.list[tl.first + i];
            require(r < t.recs.size(), cs.name, "a list entry beyond the records");
            if (i) require(r > t.list[tl.first + i - 1], cs.name, "a tile's list is not ascending");
            if (r >= t.recs.size()) continue;
            const fr::RectRec &c = t.recs[r];
            const uint64_t tx0 = 64ull * tl.x, ty0 = 64ull * tl.y;
            require(c.x0 < tx0 + 64ull * fr::LAYER_TILE_W && c.x1 > tx0 && c.y0 < ty0 + 64ull * fr::LAYER_TILE_H && c.y1 > ty0, cs.name,
                    "a tile lists a record whose bounding box does not meet it");
        }
    }
    require(next == t.list.size(), cs.name, "list entries that belong to no tile");
    for (size_t r = 0; r < t.recs.size(); ++r) {
        const fr::RectRec &c = t.recs[r];
        require(c.x0 < c.x1 && c.y0 < c.y1 && (c.rgba >> 24) != 0, cs.name, "a record that draws nothing");
        require(c.x1 <= 64ull * cs.ds && c.y1 <= 64ull * cs.dr && c.x1 <= 0x7fffffffu && c.y1 <= 0x7fffffffu, cs.name, "a record beyond the image");
        if (r) require(c.index > t.recs[r - 1].index, cs.name, "records out of the caller's order");
        listed += (size_t)(((c.x1 - 1) >> 14) - (c.x0 >> 14) + 1) * (((c.y1 - 1) >> 10) - (c.y0 >> 10) + 1);
    }
    require(listed == t.list.size(), cs.name, "a record is missing from a tile it meets");
}

}  // namespace

int main()
{
    for (const Case &cs : cases()) {
        const fr::RectsIn in{cs.dst, cs.ds, cs.dr, cs.null_rects ? nullptr : cs.rects.data(), (uint32_t)cs.rects.size(), cs.flags};
        fr::RectsTables t;
        clear_error();
        const int rc = fr::layer_rects_tables(in, t);
        std::vector<std::string> rl, cl, tl, ll;
        for (const fr_layer_rect &r : cs.rects) rl.push_back(fmt("%d,%d,%d,%d,%u,%u,%u,%u", r.x0, r.y0, r.x1, r.y1, r.rgba[0], r.rgba[1], r.rgba[2], r.rgba[3]));
        printf("%s rc=%d in=%llu,%zu,%zu,%u rects=%s%s | ", cs.name.c_str(), rc, (unsigned long long)cs.dst, cs.ds, cs.dr, cs.flags, join(rl).c_str(),
               cs.null_rects ? " null" : "");
        if (rc) {
            printf("err=%s\n", last_error());
            continue;
        }
        for (const fr::RectRec &c : t.recs) cl.push_back(fmt("%u,%u,%u,%u,%u,%u", c.x0, c.y0, c.x1, c.y1, c.rgba, c.index));
        for (const fr::RectTile &x : t.tiles) tl.push_back(fmt("%u,%u,%u,%u", x.x, x.y, x.first, x.count));
        for (const uint32_t i : t.list) ll.push_back(fmt("%u", i));
        printf("vec=%d recs=%s tiles=%s list=%s\n", t.dst_vec ? 1 : 0, join(cl).c_str(), join(tl).c_str(), join(ll).c_str());
        check_tables(cs, t);
    }
    return exit_status();
}

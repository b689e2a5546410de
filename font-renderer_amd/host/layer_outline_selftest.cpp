// layer_outline_selftest.cpp — the host side of fr_layer_outline (csrc/fr_layer_outline_plan.cpp) on the CPU: links
// fr_layer_outline_plan.o and nothing else of the library.  No GPU; the device pointers are made-up integers.  It prints one
// line per case,
//   <case> rc=<code> in=<src>,<dst>,<src stride>,<src rows>,<dst stride>,<dst rows>,<flags>
//          outline=<src_x,src_y,w,h,dst_x,dst_y,dst_w,dst_h,dx,dy,radius,kind> |
//          nothing=<0|1> zeros=<0|1> want=<x0,y0,x1,y1> live=<x0,y0,x1,y1> vec=<0|1> lead=<pixels> tiles=<x,y> reach=<R>
// or, for a refused call, "| err=<the message left>" behind the bar (outline=null: no parameters were passed), and then one
// line per radius of a list,
//   table/<rho> reach=<R> reach4=<R4> words=<per row> levels=<n> rows=<core,rim,level;...> k=<(2 R + 1)^2 weights, two hex digits each>
// tests/test_layer_outline_tables.py restates the checks, the rectangles and the weights in Python from the inputs of each
// line and compares.  After each line it checks what the kernel relies on (the live rectangle inside the wanted one, the
// tiles covering the rectangle, every row's core and rim inside the reach and its level's windows covering the core, the
// packed table decoding to the weights and to nothing else) and fails with the case and the property on stderr.
#include "../csrc/fr_layer_outline_plan.hpp"
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
    fr_layer_outline_params p;
    bool null_outline = false;
};

constexpr uintptr_t SRC = 0x10000000u, DST = 0x20000000u;

fr_layer_outline_params P(uint32_t sx, uint32_t sy, uint32_t w, uint32_t h, uint32_t x, uint32_t y, uint32_t dw, uint32_t dh, int32_t dx, int32_t dy,
                          uint32_t rho, uint32_t kind)
{
    return fr_layer_outline_params{sx, sy, w, h, x, y, dw, dh, dx, dy, rho, kind, {10, 20, 30, 200}};
}

// the layer is 300 x 50 unless a case says otherwise; the destination 132 x 60
std::vector<Case> cases()
{
    std::vector<Case> c;
    const fr_layer_outline_params ok = P(0, 0, 97, 41, 0, 0, 100, 50, 0, 0, 40, FR_OUTLINE_GROW);
    c.push_back({"typical", SRC, DST, 300, 50, 132, 60, 0, ok});
    c.push_back({"typical_srgb", SRC, DST, 300, 50, 132, 60, FR_LAYER_SRGB, ok});
    for (uint32_t kind = 0; kind < 4; ++kind) {
        c.push_back({fmt("padded_by_reach_kind%u", kind), SRC, DST, 300, 50, 132, 70, 0, P(0, 0, 97, 41, 0, 0, 103, 47, 3, 3, 40, kind)});
        c.push_back({fmt("radius_0_kind%u", kind), SRC, DST, 300, 50, 132, 60, 0, P(3, 2, 97, 41, 5, 6, 100, 50, 2, 3, 0, kind)});
        // R = 3 around the 97 x 41 window: reached by GROW and RING from 99 columns away, not from 100; INNER and SHRINK end
        // with the window
        c.push_back({fmt("just_in_reach_kind%u", kind), SRC, DST, 300, 50, 132, 60, 0, P(0, 0, 97, 41, 0, 0, 20, 20, -99, 0, 33, kind)});
        c.push_back({fmt("just_out_of_reach_kind%u", kind), SRC, DST, 300, 50, 132, 60, 0, P(0, 0, 97, 41, 0, 0, 20, 20, -100, 0, 33, kind)});
        c.push_back({fmt("last_window_column_kind%u", kind), SRC, DST, 300, 50, 132, 60, 0, P(0, 0, 97, 41, 0, 0, 20, 20, -96, 0, 33, kind)});
        c.push_back({fmt("first_column_beyond_kind%u", kind), SRC, DST, 300, 50, 132, 60, 0, P(0, 0, 97, 41, 0, 0, 20, 20, -97, 0, 33, kind)});
        c.push_back({fmt("in_reach_above_kind%u", kind), SRC, DST, 300, 50, 132, 60, 0, P(0, 0, 97, 41, 0, 0, 20, 20, 0, 22, 33, kind)});
        c.push_back({fmt("out_of_reach_above_kind%u", kind), SRC, DST, 300, 50, 132, 60, 0, P(0, 0, 97, 41, 0, 0, 20, 20, 0, 23, 33, kind)});
        c.push_back({fmt("zero_window_width_kind%u", kind), SRC, DST, 300, 50, 132, 60, 0, P(1000, 1000, 0, 41, 0, 0, 100, 50, 0, 0, 40, kind)});
    }
    c.push_back({"radius_1", SRC, DST, 300, 50, 132, 60, 0, P(0, 0, 97, 41, 0, 0, 100, 50, 0, 0, 1, FR_OUTLINE_RING)});
    c.push_back({"radius_16", SRC, DST, 300, 50, 132, 60, 0, P(0, 0, 97, 41, 0, 0, 100, 50, 0, 0, 16, FR_OUTLINE_RING)});
    c.push_back({"radius_17", SRC, DST, 300, 50, 132, 60, 0, P(0, 0, 97, 41, 0, 0, 100, 50, 0, 0, 17, FR_OUTLINE_INNER)});
    c.push_back({"radius_256", SRC, DST, 300, 50, 132, 60, 0, P(0, 0, 97, 41, 0, 0, 132, 60, -3, 4, 256, FR_OUTLINE_SHRINK)});
    c.push_back({"radius_257", SRC, DST, 300, 50, 132, 60, 0, P(0, 0, 97, 41, 0, 0, 100, 50, 0, 0, 257, FR_OUTLINE_GROW)});
    c.push_back({"kind_4", SRC, DST, 300, 50, 132, 60, 0, P(0, 0, 97, 41, 0, 0, 100, 50, 0, 0, 40, 4)});
    c.push_back({"radius_before_kind", SRC, DST, 300, 50, 132, 60, 0, P(0, 0, 97, 41, 0, 0, 100, 50, 0, 0, 300, 9)});
    c.push_back({"small_rect_in_a_large_window", SRC, DST, 300, 50, 132, 60, 0, P(0, 0, 300, 50, 40, 20, 9, 5, -100, -10, 100, FR_OUTLINE_GROW)});
    c.push_back({"cut_left_and_top", SRC, DST, 300, 50, 132, 60, 0, P(0, 0, 97, 41, 0, 0, 60, 30, -20, -15, 40, FR_OUTLINE_RING)});
    c.push_back({"cut_right_and_bottom", SRC, DST, 300, 50, 132, 60, 0, P(0, 0, 97, 41, 4, 4, 80, 35, 40, 20, 40, FR_OUTLINE_GROW)});
    c.push_back({"inner_cut_to_the_window", SRC, DST, 300, 50, 132, 70, 0, P(0, 0, 97, 41, 0, 0, 132, 70, 10, 12, 256, FR_OUTLINE_INNER)});
    c.push_back({"offset_int32_min", SRC, DST, 300, 50, 132, 60, 0, P(0, 0, 97, 41, 0, 0, 100, 50, INT32_MIN, INT32_MIN, 256, FR_OUTLINE_GROW)});
    c.push_back({"offset_int32_max", SRC, DST, 300, 50, 132, 60, 0, P(0, 0, 97, 41, 0, 0, 100, 50, INT32_MAX, INT32_MAX, 256, FR_OUTLINE_GROW)});
    c.push_back({"zero_window_height", SRC, DST, 300, 50, 132, 60, 0, P(0, 0, 97, 0, 0, 0, 100, 50, 0, 0, 40, FR_OUTLINE_SHRINK)});
    c.push_back({"zero_rect_width", SRC, DST, 300, 50, 132, 60, 0, P(0, 0, 97, 41, 1000, 1000, 0, 50, 0, 0, 40, FR_OUTLINE_GROW)});
    c.push_back({"zero_rect_height", SRC, DST, 300, 50, 132, 60, 0, P(0, 0, 97, 41, 0, 0, 100, 0, 0, 0, 40, FR_OUTLINE_GROW)});
    c.push_back({"zero_rect_bad_radius", SRC, DST, 300, 50, 132, 60, 0, P(0, 0, 97, 41, 0, 0, 100, 0, 0, 0, 257, FR_OUTLINE_GROW)});
    c.push_back({"one_by_one", SRC, DST, 300, 50, 132, 60, 0, P(7, 7, 1, 1, 0, 0, 21, 21, 10, 10, 160, FR_OUTLINE_GROW)});
    c.push_back({"window_last_column_in", SRC, DST, 300, 50, 132, 60, 0, P(203, 9, 97, 41, 0, 0, 100, 50, 0, 0, 40, FR_OUTLINE_GROW)});
    c.push_back({"window_one_pixel_out_right", SRC, DST, 300, 50, 132, 60, 0, P(204, 9, 97, 41, 0, 0, 100, 50, 0, 0, 40, FR_OUTLINE_GROW)});
    c.push_back({"window_one_pixel_out_below", SRC, DST, 300, 50, 132, 60, 0, P(203, 10, 97, 41, 0, 0, 100, 50, 0, 0, 40, FR_OUTLINE_GROW)});
    c.push_back({"rect_last_column_and_row_in", SRC, DST, 300, 50, 132, 60, 0, P(0, 0, 97, 41, 32, 10, 100, 50, 0, 0, 40, FR_OUTLINE_GROW)});
    c.push_back({"rect_one_pixel_out_right", SRC, DST, 300, 50, 132, 60, 0, P(0, 0, 97, 41, 33, 10, 100, 50, 0, 0, 40, FR_OUTLINE_GROW)});
    c.push_back({"rect_one_pixel_out_below", SRC, DST, 300, 50, 132, 60, 0, P(0, 0, 97, 41, 32, 11, 100, 50, 0, 0, 40, FR_OUTLINE_GROW)});
    c.push_back({"rect_x_wraps_32_bits", SRC, DST, 300, 50, 132, 60, 0, P(0, 0, 97, 41, 0xffffffffu, 0, 2, 50, 0, 0, 40, FR_OUTLINE_GROW)});
    c.push_back({"window_before_radius", SRC, DST, 300, 50, 132, 60, 0, P(204, 9, 97, 41, 0, 0, 100, 50, 0, 0, 257, FR_OUTLINE_GROW)});
    c.push_back({"src_null", 0, DST, 300, 50, 132, 60, 0, ok});
    c.push_back({"dst_null", SRC, 0, 300, 50, 132, 60, 0, ok});
    c.push_back({"outline_null", SRC, DST, 300, 50, 132, 60, 0, ok, true});
    c.push_back({"src_not_4_aligned", SRC + 2, DST, 300, 50, 132, 60, 0, ok});
    c.push_back({"dst_not_4_aligned", SRC, DST + 1, 300, 50, 132, 60, 0, ok});
    // the stores: rows of 132 pixels on the 16-byte grid, the rectangle's first pixel 0 .. 3 pixels off it; rows of 131 not
    c.push_back({"lead_0", SRC, DST, 300, 50, 132, 60, 0, P(0, 0, 97, 41, 4, 1, 60, 50, 0, 0, 40, FR_OUTLINE_GROW)});
    c.push_back({"lead_1", SRC, DST, 300, 50, 132, 60, 0, P(0, 0, 97, 41, 5, 1, 60, 50, 0, 0, 40, FR_OUTLINE_GROW)});
    c.push_back({"lead_3_adds_a_tile_column", SRC, DST, 300, 50, 132, 60, 0, P(0, 0, 97, 41, 3, 1, 62, 50, 0, 0, 40, FR_OUTLINE_GROW)});
    c.push_back({"lead_from_the_pointer", SRC, DST + 12, 300, 50, 132, 60, 0, P(0, 0, 97, 41, 0, 0, 62, 50, 0, 0, 40, FR_OUTLINE_GROW)});
    c.push_back({"rows_of_131", SRC, DST, 300, 50, 131, 60, 0, P(0, 0, 97, 41, 3, 1, 62, 50, 0, 0, 40, FR_OUTLINE_GROW)});
    c.push_back({"unknown_flag_2", SRC, DST, 300, 50, 132, 60, 2, ok});
    c.push_back({"text_flag_bits", SRC, DST, 300, 50, 132, 60, FR_TEXT_SRGB | FR_TEXT_OVER, ok});
    c.push_back({"flag_before_null", 0, 0, 300, 50, 132, 60, 4, ok, true});
    c.push_back({"aliasing_same_image", SRC, SRC, 300, 50, 300, 50, 0, P(0, 0, 97, 41, 100, 0, 100, 50, 0, 0, 40, FR_OUTLINE_GROW)});
    c.push_back({"aliasing_last_byte", SRC, SRC + 4 * 300 * 50 - 4, 300, 50, 132, 60, 0, ok});
    c.push_back({"adjacent_images", SRC, SRC + 4 * 300 * 50, 300, 50, 132, 60, 0, ok});
    c.push_back({"radius_before_aliasing", SRC, SRC, 300, 50, 300, 50, 0, P(0, 0, 97, 41, 100, 0, 100, 50, 0, 0, 257, FR_OUTLINE_GROW)});
    c.push_back({"src_pitch_max", (uintptr_t)1 << 40, DST, (size_t)1 << 26, 3, 132, 60, 0, P((1u << 26) - 97, 0, 97, 3, 0, 0, 100, 50, 0, 0, 40, FR_OUTLINE_GROW)});
    c.push_back({"src_pitch_over", (uintptr_t)1 << 40, DST, ((size_t)1 << 26) + 1, 3, 132, 60, 0, ok});
    c.push_back({"dst_pitch_max", SRC, (uintptr_t)1 << 40, 300, 50, (size_t)1 << 26, 3, 0, P(0, 0, 97, 41, (1u << 26) - 100, 0, 100, 3, 0, 0, 40, FR_OUTLINE_GROW)});
    c.push_back({"dst_pitch_over", SRC, (uintptr_t)1 << 40, 300, 50, ((size_t)1 << 26) + 1, 3, 0, ok});
    c.push_back({"src_rows_max", (uintptr_t)1 << 44, DST, 4, 0x7fffffffu, 132, 60, 0, P(0, 0x7fffffffu - 41, 4, 41, 0, 0, 100, 50, 0, 0, 40, FR_OUTLINE_GROW)});
    c.push_back({"src_rows_over", (uintptr_t)1 << 44, DST, 4, (size_t)1 << 31, 132, 60, 0, ok});
    c.push_back({"dst_rows_max", SRC, (uintptr_t)1 << 44, 300, 50, 4, 0x7fffffffu, 0, P(0, 0, 97, 41, 0, 0x7fffffffu - 50, 4, 50, 0, 0, 40, FR_OUTLINE_GROW)});
    c.push_back({"dst_rows_over", SRC, (uintptr_t)1 << 44, 300, 50, 4, (size_t)1 << 31, 0, ok});
    // the destination rectangle's tiles: (131069 + 3) / 64 = 2048 columns of tiles by 2048 rows is 2^22
    c.push_back({"rect_tiles_at_2_22", (uintptr_t)1 << 44, (uintptr_t)1 << 52, 1u << 20, 1u << 20, 1u << 18, 1u << 18, 0,
                 P(0, 0, 1u << 20, 1u << 20, 0, 0, 131069, 131072, 0, 0, 256, FR_OUTLINE_GROW)});
    c.push_back({"rect_tiles_over_by_a_column", (uintptr_t)1 << 44, (uintptr_t)1 << 52, 1u << 20, 1u << 20, 1u << 18, 1u << 18, 0,
                 P(0, 0, 1u << 20, 1u << 20, 0, 0, 131070, 131072, 0, 0, 256, FR_OUTLINE_GROW)});
    c.push_back({"rect_tiles_over_by_a_row", (uintptr_t)1 << 44, (uintptr_t)1 << 52, 1u << 20, 1u << 20, 1u << 18, 1u << 18, 0,
                 P(0, 0, 1u << 20, 1u << 20, 0, 0, 131069, 131073, 0, 0, 0, FR_OUTLINE_GROW)});
    c.push_back({"rect_tiles_over_out_of_reach", (uintptr_t)1 << 44, (uintptr_t)1 << 52, 1u << 20, 1u << 20, 1u << 26, 1u << 30, 0,
                 P(0, 0, 10, 10, 0, 0, 1u << 26, 1u << 30, -1000, 0, 256, FR_OUTLINE_GROW)});
    return c;
}

bool inside(const fr::ShadowRect &a, const fr::ShadowRect &b) { return a.x0 >= b.x0 && a.y0 >= b.y0 && a.x1 <= b.x1 && a.y1 <= b.y1; }

// what the kernel relies on in a table
void check_table(const std::string &name, uint32_t rho, const fr::OutlineTable &t)
{
    const uint32_t n = 2 * t.reach + 1;
    require(t.reach == fr::outline_reach(rho) && t.reach <= fr::OUTLINE_MAX_REACH && t.reach4 % 4 == 0 && t.reach4 >= t.reach && t.reach4 < t.reach + 4, name,
            "the reach or its rounding");
    require(t.row_words == t.reach4 / 2 + 1, name, "the words of a row");
    require(t.rows.size() == n && t.k.size() == (size_t)n * n, name, "the table's sizes");
    require(t.packed.size() % 4 == 0 && t.packed.size() >= 4 * (size_t)n + (size_t)n * t.row_words, name, "the packed table is too small");
    if (exit_status()) return;
    const uint32_t *w = t.packed.data() + 4 * (size_t)n;
    for (uint32_t jj = 0; jj < n; ++jj) {
        const fr::OutlineRow &r = t.rows[jj];
        require(r.core <= (int32_t)t.reach && r.core + (int32_t)r.rim <= (int32_t)t.reach, name, "a row's core and rim leave the reach");
        require(r.level <= t.levels && t.levels <= 5, name, "a row's level beyond the table's levels");
        require(r.core < 0 ? r.level == 0 : (1u << r.level) <= 2u * (uint32_t)r.core + 1u, name, "a window of the row's level is wider than its core");
        require(r.core < 0 || (2u << r.level) > 2u * (uint32_t)r.core + 1u, name, "two windows of the row's level do not cover its core");
        require(t.packed[4 * jj] == (uint32_t)r.core && t.packed[4 * jj + 1] == r.rim && t.packed[4 * jj + 2] == r.level && t.packed[4 * jj + 3] == 0u, name,
                "a packed row record");
        for (uint32_t tap = 0; tap < 4 * t.row_words; ++tap) {
            const int32_t i = (int32_t)tap - (int32_t)t.reach4;
            const uint32_t got = (w[jj * t.row_words + tap / 4] >> (8 * (tap % 4))) & 0xffu;
            const uint32_t want = (uint32_t)std::abs(i) <= t.reach ? t.k[(size_t)jj * n + (uint32_t)(i + (int32_t)t.reach)] : 0u;
            require(got == want, name, "a packed weight");
            const int32_t d = std::abs(i);
            require(d <= r.core ? got == 255u : d <= r.core + (int32_t)r.rim ? got > 0u && got < 255u : got == 0u, name, "a weight against the row's core and rim");
        }
    }
}

void check_plan(const Case &cs, const fr::OutlinePlan &p)
{
    if (p.nothing || p.zeros) {
        require(p.table.packed.empty() && p.live.empty(), cs.name, "a table without anything to draw");
        return;
    }
    require(!p.live.empty() && inside(p.live, p.want), cs.name, "the live rectangle leaves the wanted one");
    require(p.lead < 4 && (p.vec || !p.lead), cs.name, "the lead");
    require(p.tiles_x * fr::SHADOW_TILE >= (uint64_t)cs.p.dst_w + p.lead && p.tiles_y * fr::SHADOW_TILE >= cs.p.dst_h, cs.name, "the tiles do not cover the rectangle");
    require(p.tiles_x * p.tiles_y <= fr::SHADOW_MAX_TILES, cs.name, "too many tiles");
    check_table(cs.name, cs.p.radius, p.table);
}

}  // namespace

int main()
{
    for (const Case &cs : cases()) {
        const fr::OutlineIn in{cs.src, cs.dst, cs.ss, cs.sr, cs.ds, cs.dr, cs.null_outline ? nullptr : &cs.p, cs.flags};
        fr::OutlinePlan p;
        clear_error();
        const int rc = fr::outline_plan(in, p);
        const fr_layer_outline_params &s = cs.p;
        printf("%s rc=%d in=%llu,%llu,%zu,%zu,%zu,%zu,%u outline=%s | ", cs.name.c_str(), rc, (unsigned long long)cs.src, (unsigned long long)cs.dst, cs.ss,
               cs.sr, cs.ds, cs.dr, cs.flags,
               cs.null_outline ? "null"
                               : fmt("%u,%u,%u,%u,%u,%u,%u,%u,%d,%d,%u,%u", s.src_x, s.src_y, s.w, s.h, s.dst_x, s.dst_y, s.dst_w, s.dst_h, s.dx, s.dy, s.radius,
                                     s.kind).c_str());
        if (rc) {
            printf("err=%s\n", last_error());
            continue;
        }
        printf("nothing=%d zeros=%d want=%lld,%lld,%lld,%lld live=%lld,%lld,%lld,%lld vec=%u lead=%u tiles=%llu,%llu reach=%u\n", p.nothing ? 1 : 0,
               p.zeros ? 1 : 0, (long long)p.want.x0, (long long)p.want.y0, (long long)p.want.x1, (long long)p.want.y1, (long long)p.live.x0,
               (long long)p.live.y0, (long long)p.live.x1, (long long)p.live.y1, p.vec, p.lead, (unsigned long long)p.tiles_x, (unsigned long long)p.tiles_y,
               p.table.reach);
        check_plan(cs, p);
    }
    for (uint32_t rho : {0u, 1u, 8u, 15u, 16u, 17u, 24u, 40u, 64u, 100u, 128u, 255u, 256u}) {
        fr::OutlineTable t;
        fr::outline_table(rho, t);
        std::string rows, k;
        for (const fr::OutlineRow &r : t.rows) rows += (rows.empty() ? "" : ";") + fmt("%d,%u,%u", r.core, r.rim, r.level);
        for (uint8_t v : t.k) k += fmt("%02x", v);
        printf("table/%u reach=%u reach4=%u words=%u levels=%u rows=%s k=%s\n", rho, t.reach, t.reach4, t.row_words, t.levels, rows.c_str(), k.c_str());
        check_table(fmt("table/%u", rho), rho, t);
    }
    return exit_status();
}

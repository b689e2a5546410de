// layer_shadow_selftest.cpp — the host side of fr_layer_shadow (csrc/fr_layer_shadow_plan.cpp) on the CPU: links
// fr_layer_shadow_plan.o and nothing else of the library.  No GPU; the device pointers are made-up integers.  It prints one
// line per case,
//   <case> rc=<code> in=<src>,<dst>,<src stride>,<src rows>,<dst stride>,<dst rows>,<flags>
//          shadow=<src_x,src_y,w,h,dst_x,dst_y,dst_w,dst_h,dx,dy,s,r,p> |
//          nothing=<0|1> zeros=<0|1> want=<x0,y0,x1,y1> planes=<bytes,bytes> stages=<kind,radius,x0,y0,x1,y1,pitch,m,shift;...>
// or, for a refused call, "| err=<the message left>" behind the bar (shadow=null: no parameters were passed), and then one
// line "recip/<r> m=<m> shift=<shift>" per blur radius.  tests/test_layer_shadow_tables.py restates the checks and the
// rectangles in Python from the inputs of each line and compares.  After each line it checks what the kernels rely on
// (every stage's rectangle inside its input's rectangle grown by the radius, a plane large enough for it) and fails with the
// case and the property on stderr.
#include "../csrc/fr_layer_shadow_plan.hpp"
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
    fr_layer_shadow_params p;
    bool null_shadow = false;
};

constexpr uintptr_t SRC = 0x10000000u, DST = 0x20000000u;

fr_layer_shadow_params P(uint32_t sx, uint32_t sy, uint32_t w, uint32_t h, uint32_t x, uint32_t y, uint32_t dw, uint32_t dh, int32_t dx, int32_t dy,
                         uint32_t s, uint32_t r, uint32_t p)
{
    return fr_layer_shadow_params{sx, sy, w, h, x, y, dw, dh, dx, dy, s, r, p, {10, 20, 30, 200}};
}

// the layer is 300 x 50 unless a case says otherwise; the destination 132 x 60
std::vector<Case> cases()
{
    std::vector<Case> c;
    const fr_layer_shadow_params ok = P(0, 0, 97, 41, 0, 0, 100, 50, 0, 0, 1, 3, 3);
    c.push_back({"typical", SRC, DST, 300, 50, 132, 60, 0, ok});
    c.push_back({"typical_srgb", SRC, DST, 300, 50, 132, 60, FR_LAYER_SRGB, ok});
    c.push_back({"padded_by_reach", SRC, DST, 300, 50, 132, 70, 0, P(0, 0, 97, 41, 0, 0, 117, 61, 10, 10, 1, 3, 3)});
    c.push_back({"no_stage", SRC, DST, 300, 50, 132, 60, 0, P(3, 2, 97, 41, 5, 6, 100, 50, 2, 3, 0, 0, 0)});
    c.push_back({"radius_without_passes", SRC, DST, 300, 50, 132, 60, 0, P(0, 0, 97, 41, 0, 0, 100, 50, 0, 0, 0, 7, 0)});
    c.push_back({"passes_without_radius", SRC, DST, 300, 50, 132, 60, 0, P(0, 0, 97, 41, 0, 0, 100, 50, 0, 0, 0, 0, 3)});
    c.push_back({"spread_only", SRC, DST, 300, 50, 132, 60, 0, P(0, 0, 97, 41, 0, 0, 100, 50, 0, 0, 2, 0, 0)});
    c.push_back({"one_box", SRC, DST, 300, 50, 132, 60, 0, P(0, 0, 97, 41, 0, 0, 100, 50, 0, 0, 0, 32, 1)});
    c.push_back({"limits_8_32_3", SRC, DST, 300, 50, 132, 60, 0, P(0, 0, 97, 41, 0, 0, 132, 60, -3, 4, 8, 32, 3)});
    c.push_back({"spread_9", SRC, DST, 300, 50, 132, 60, 0, P(0, 0, 97, 41, 0, 0, 100, 50, 0, 0, 9, 32, 3)});
    c.push_back({"radius_33", SRC, DST, 300, 50, 132, 60, 0, P(0, 0, 97, 41, 0, 0, 100, 50, 0, 0, 8, 33, 3)});
    c.push_back({"passes_4", SRC, DST, 300, 50, 132, 60, 0, P(0, 0, 97, 41, 0, 0, 100, 50, 0, 0, 8, 32, 4)});
    c.push_back({"radius_33_without_passes", SRC, DST, 300, 50, 132, 60, 0, P(0, 0, 97, 41, 0, 0, 100, 50, 0, 0, 0, 33, 0)});
    c.push_back({"small_rect_in_a_large_window", SRC, DST, 300, 50, 132, 60, 0, P(0, 0, 300, 50, 40, 20, 9, 5, -100, -10, 2, 4, 2)});
    c.push_back({"cut_left_and_top", SRC, DST, 300, 50, 132, 60, 0, P(0, 0, 97, 41, 0, 0, 60, 30, -20, -15, 1, 3, 2)});
    c.push_back({"negative_offset_beyond_the_window", SRC, DST, 300, 50, 132, 60, 0, P(0, 0, 97, 41, 0, 0, 100, 50, -90, 0, 0, 4, 2)});
    c.push_back({"just_in_reach", SRC, DST, 300, 50, 132, 60, 0, P(0, 0, 97, 41, 0, 0, 20, 20, -106, 0, 1, 3, 3)});
    c.push_back({"just_out_of_reach", SRC, DST, 300, 50, 132, 60, 0, P(0, 0, 97, 41, 0, 0, 20, 20, -107, 0, 1, 3, 3)});
    c.push_back({"out_of_reach_above", SRC, DST, 300, 50, 132, 60, 0, P(0, 0, 97, 41, 0, 0, 20, 20, 0, 30, 1, 3, 3)});
    c.push_back({"in_reach_above", SRC, DST, 300, 50, 132, 60, 0, P(0, 0, 97, 41, 0, 0, 20, 20, 0, 29, 1, 3, 3)});
    c.push_back({"offset_int32_min", SRC, DST, 300, 50, 132, 60, 0, P(0, 0, 97, 41, 0, 0, 100, 50, INT32_MIN, INT32_MIN, 1, 3, 3)});
    c.push_back({"offset_int32_max", SRC, DST, 300, 50, 132, 60, 0, P(0, 0, 97, 41, 0, 0, 100, 50, INT32_MAX, INT32_MAX, 1, 3, 3)});
    c.push_back({"zero_window_width", SRC, DST, 300, 50, 132, 60, 0, P(1000, 1000, 0, 41, 0, 0, 100, 50, 0, 0, 1, 3, 3)});
    c.push_back({"zero_window_height", SRC, DST, 300, 50, 132, 60, 0, P(0, 0, 97, 0, 0, 0, 100, 50, 0, 0, 1, 3, 3)});
    c.push_back({"zero_rect_width", SRC, DST, 300, 50, 132, 60, 0, P(0, 0, 97, 41, 1000, 1000, 0, 50, 0, 0, 1, 3, 3)});
    c.push_back({"zero_rect_height", SRC, DST, 300, 50, 132, 60, 0, P(0, 0, 97, 41, 0, 0, 100, 0, 0, 0, 1, 3, 3)});
    c.push_back({"one_by_one", SRC, DST, 300, 50, 132, 60, 0, P(7, 7, 1, 1, 0, 0, 21, 21, 10, 10, 0, 5, 2)});
    c.push_back({"window_last_column_in", SRC, DST, 300, 50, 132, 60, 0, P(203, 9, 97, 41, 0, 0, 100, 50, 0, 0, 1, 3, 3)});
    c.push_back({"window_one_pixel_out_right", SRC, DST, 300, 50, 132, 60, 0, P(204, 9, 97, 41, 0, 0, 100, 50, 0, 0, 1, 3, 3)});
    c.push_back({"window_one_pixel_out_below", SRC, DST, 300, 50, 132, 60, 0, P(203, 10, 97, 41, 0, 0, 100, 50, 0, 0, 1, 3, 3)});
    c.push_back({"rect_last_column_and_row_in", SRC, DST, 300, 50, 132, 60, 0, P(0, 0, 97, 41, 32, 10, 100, 50, 0, 0, 1, 3, 3)});
    c.push_back({"rect_one_pixel_out_right", SRC, DST, 300, 50, 132, 60, 0, P(0, 0, 97, 41, 33, 10, 100, 50, 0, 0, 1, 3, 3)});
    c.push_back({"rect_one_pixel_out_below", SRC, DST, 300, 50, 132, 60, 0, P(0, 0, 97, 41, 32, 11, 100, 50, 0, 0, 1, 3, 3)});
    c.push_back({"rect_x_wraps_32_bits", SRC, DST, 300, 50, 132, 60, 0, P(0, 0, 97, 41, 0xffffffffu, 0, 2, 50, 0, 0, 1, 3, 3)});
    c.push_back({"src_null", 0, DST, 300, 50, 132, 60, 0, ok});
    c.push_back({"dst_null", SRC, 0, 300, 50, 132, 60, 0, ok});
    c.push_back({"shadow_null", SRC, DST, 300, 50, 132, 60, 0, ok, true});
    c.push_back({"src_not_4_aligned", SRC + 2, DST, 300, 50, 132, 60, 0, ok});
    c.push_back({"dst_not_4_aligned", SRC, DST + 1, 300, 50, 132, 60, 0, ok});
    c.push_back({"both_4_aligned_only", SRC + 4, DST + 12, 300, 50, 132, 60, 0, ok});
    c.push_back({"unknown_flag_2", SRC, DST, 300, 50, 132, 60, 2, ok});
    c.push_back({"text_flag_bits", SRC, DST, 300, 50, 132, 60, FR_TEXT_SRGB | FR_TEXT_OVER, ok});
    c.push_back({"flag_before_null", 0, 0, 300, 50, 132, 60, 4, ok, true});
    c.push_back({"aliasing_same_image", SRC, SRC, 300, 50, 300, 50, 0, P(0, 0, 97, 41, 100, 0, 100, 50, 0, 0, 1, 3, 3)});
    c.push_back({"aliasing_last_byte", SRC, SRC + 4 * 300 * 50 - 4, 300, 50, 132, 60, 0, ok});
    c.push_back({"adjacent_images", SRC, SRC + 4 * 300 * 50, 300, 50, 132, 60, 0, ok});
    c.push_back({"src_pitch_max", (uintptr_t)1 << 40, DST, (size_t)1 << 26, 3, 132, 60, 0, P((1u << 26) - 97, 0, 97, 3, 0, 0, 100, 50, 0, 0, 1, 3, 3)});
    c.push_back({"src_pitch_over", (uintptr_t)1 << 40, DST, ((size_t)1 << 26) + 1, 3, 132, 60, 0, ok});
    c.push_back({"dst_pitch_max", SRC, (uintptr_t)1 << 40, 300, 50, (size_t)1 << 26, 3, 0, P(0, 0, 97, 41, (1u << 26) - 100, 0, 100, 3, 0, 0, 1, 3, 3)});
    c.push_back({"dst_pitch_over", SRC, (uintptr_t)1 << 40, 300, 50, ((size_t)1 << 26) + 1, 3, 0, ok});
    c.push_back({"src_rows_max", (uintptr_t)1 << 44, DST, 4, 0x7fffffffu, 132, 60, 0, P(0, 0x7fffffffu - 41, 4, 41, 0, 0, 100, 50, 0, 0, 1, 3, 3)});
    c.push_back({"src_rows_over", (uintptr_t)1 << 44, DST, 4, (size_t)1 << 31, 132, 60, 0, ok});
    c.push_back({"dst_rows_max", SRC, (uintptr_t)1 << 44, 300, 50, 4, 0x7fffffffu, 0, P(0, 0, 97, 41, 0, 0x7fffffffu - 50, 4, 50, 0, 0, 1, 3, 3)});
    c.push_back({"dst_rows_over", SRC, (uintptr_t)1 << 44, 300, 50, 4, (size_t)1 << 31, 0, ok});
    // the planes of three passes of radius 16 well inside a large window: 16320 + 64 and 16320 + 32 columns, 16384 bytes a row
    // both, by H + 64 and H + 32 rows: 2^30 bytes together at H = 32720
    c.push_back({"planes_at_2_30", (uintptr_t)1 << 44, (uintptr_t)1 << 48, 1u << 20, 1u << 20, 1u << 20, 1u << 20, 0,
                 P(0, 0, 1u << 20, 1u << 20, 0, 0, 16320, 32720, -100, -100, 0, 16, 3)});
    c.push_back({"planes_over_2_30", (uintptr_t)1 << 44, (uintptr_t)1 << 48, 1u << 20, 1u << 20, 1u << 20, 1u << 20, 0,
                 P(0, 0, 1u << 20, 1u << 20, 0, 0, 16320, 32721, -100, -100, 0, 16, 3)});
    // the destination rectangle's tiles: (131069 + 3) / 64 = 2048 columns of tiles by 2048 rows is 2^22; one stage has no plane
    c.push_back({"rect_tiles_at_2_22", (uintptr_t)1 << 44, (uintptr_t)1 << 52, 1u << 20, 1u << 20, 1u << 18, 1u << 18, 0,
                 P(0, 0, 1u << 20, 1u << 20, 0, 0, 131069, 131072, 0, 0, 8, 0, 0)});
    c.push_back({"rect_tiles_over_by_a_column", (uintptr_t)1 << 44, (uintptr_t)1 << 52, 1u << 20, 1u << 20, 1u << 18, 1u << 18, 0,
                 P(0, 0, 1u << 20, 1u << 20, 0, 0, 131070, 131072, 0, 0, 8, 0, 0)});
    c.push_back({"rect_tiles_over_by_a_row", (uintptr_t)1 << 44, (uintptr_t)1 << 52, 1u << 20, 1u << 20, 1u << 18, 1u << 18, 0,
                 P(0, 0, 1u << 20, 1u << 20, 0, 0, 131069, 131073, 0, 0, 0, 0, 0)});
    c.push_back({"rect_tiles_over_out_of_reach", (uintptr_t)1 << 44, (uintptr_t)1 << 52, 1u << 20, 1u << 20, 1u << 26, 1u << 30, 0,
                 P(0, 0, 10, 10, 0, 0, 1u << 26, 1u << 30, -1000, 0, 8, 0, 0)});
    return c;
}

bool inside(const fr::ShadowRect &a, const fr::ShadowRect &b) { return a.x0 >= b.x0 && a.y0 >= b.y0 && a.x1 <= b.x1 && a.y1 <= b.y1; }

// what the kernels rely on
void check_plan(const Case &cs, const fr::ShadowPlan &p)
{
    if (p.nothing || p.zeros) {
        require(p.stages.empty() && !p.plane_bytes[0] && !p.plane_bytes[1], cs.name, "stages without anything to draw");
        return;
    }
    fr::ShadowRect in{0, 0, (int64_t)cs.p.w, (int64_t)cs.p.h};
    for (size_t k = 0; k < p.stages.size(); ++k) {
        const fr::ShadowStage &st = p.stages[k];
        const int64_t r = st.radius;
        require(!st.out.empty(), cs.name, "an empty stage rectangle");
        require(inside(st.out, fr::ShadowRect{in.x0 - r, in.y0 - r, in.x1 + r, in.y1 + r}), cs.name, "a stage rectangle beyond its input grown by the radius");
        if (k + 1 < p.stages.size()) {
            require(st.pitch % fr::SHADOW_TILE == 0 && st.pitch >= st.out.w(), cs.name, "a plane pitch that is no whole number of tiles");
            require(st.pitch * st.out.h() <= p.plane_bytes[k & 1], cs.name, "a plane too small for its stage");
        } else {
            require(inside(st.out, p.want), cs.name, "the last rectangle leaves the destination rectangle");
        }
        in = st.out;
    }
}

}  // namespace

int main()
{
    for (const Case &cs : cases()) {
        const fr::ShadowIn in{cs.src, cs.dst, cs.ss, cs.sr, cs.ds, cs.dr, cs.null_shadow ? nullptr : &cs.p, cs.flags};
        fr::ShadowPlan p;
        clear_error();
        const int rc = fr::shadow_plan(in, p);
        const fr_layer_shadow_params &s = cs.p;
        printf("%s rc=%d in=%llu,%llu,%zu,%zu,%zu,%zu,%u shadow=%s | ", cs.name.c_str(), rc, (unsigned long long)cs.src, (unsigned long long)cs.dst, cs.ss,
               cs.sr, cs.ds, cs.dr, cs.flags,
               cs.null_shadow ? "null"
                              : fmt("%u,%u,%u,%u,%u,%u,%u,%u,%d,%d,%u,%u,%u", s.src_x, s.src_y, s.w, s.h, s.dst_x, s.dst_y, s.dst_w, s.dst_h, s.dx, s.dy, s.spread,
                                    s.blur_radius, s.blur_passes).c_str());
        if (rc) {
            printf("err=%s\n", last_error());
            continue;
        }
        std::string st;
        for (const fr::ShadowStage &x : p.stages)
            st += (st.empty() ? "" : ";") + fmt("%u,%u,%lld,%lld,%lld,%lld,%llu,%u,%u", (unsigned)x.kind, x.radius, (long long)x.out.x0, (long long)x.out.y0,
                                                (long long)x.out.x1, (long long)x.out.y1, (unsigned long long)x.pitch, x.recip.m, x.recip.shift);
        printf("nothing=%d zeros=%d want=%lld,%lld,%lld,%lld planes=%llu,%llu stages=%s\n", p.nothing ? 1 : 0, p.zeros ? 1 : 0, (long long)p.want.x0,
               (long long)p.want.y0, (long long)p.want.x1, (long long)p.want.y1, (unsigned long long)p.plane_bytes[0], (unsigned long long)p.plane_bytes[1],
               st.empty() ? "-" : st.c_str());
        check_plan(cs, p);
    }
    for (uint32_t r = 1; r <= fr::SHADOW_MAX_RADIUS; ++r) {
        const fr::ShadowRecip q = fr::shadow_recip(r);
        printf("recip/%u m=%u shift=%u\n", r, q.m, q.shift);
    }
    return exit_status();
}

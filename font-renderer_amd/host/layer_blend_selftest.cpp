// layer_blend_selftest.cpp — the arithmetic and the checks of fr_layer_blend (csrc/fr_layer_blend_math.hpp) on the CPU: the
// text the kernel compiles, compiled here as plain C++.  Links fr_layer_plan.o and nothing else of the library.  No GPU.
//   div255 checked=<n> bad=<n>                    blend_div255 against n / 255 for every n below 2^24
//   div65535 checked=<n> bad=<n> top=<n>          blend_div65535 against n / 65535 at every multiple of 65535, one below and
//                                                 one above, up to 3 * 65535^2 + 65535, and at 2^20 multiples spread up to 2^47
//   px/<Q>/<mode> corners=<n> random=<n> bad=<n> valid_over=<n> digest=<d>
//                                                 blend_channel against a restatement in 64-bit integers, on the corners of
//                                                 (x, y, p, q) and on random values; valid_over: valid premultiplied inputs
//                                                 whose N exceeds Q^2 (must be 0); digest: over the outputs of a fixed
//                                                 sequence of inputs, which tests/test_layer_blend_ref.py draws again for the twin
//   check/<case> rc=<code> | err=<message> or tiles=<n>
// A bad count above 0 fails the program with the property on stderr.
#include "../csrc/fr_layer_blend_math.hpp"
#include "selftest.hpp"

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <vector>

using namespace selftest;

namespace {

const char *const MODE_NAME[FR_BLEND_MODES] = {"multiply", "screen", "overlay", "darken", "lighten", "hard_light", "difference", "exclusion", "plus"};

// the header's definition, every term a signed 64-bit integer: N, and out with the language's own division
int64_t restated_n(uint32_t mode, int64_t Q, int64_t x, int64_t y, int64_t p, int64_t q)
{
    const auto pos = [](int64_t v) { return std::max<int64_t>(v, 0); };
    const int64_t light = pos(p * q - 2 * pos(q - y) * pos(p - x));
    int64_t b2 = 0;
    switch (mode) {
    case FR_BLEND_MULTIPLY: b2 = x * y; break;
    case FR_BLEND_SCREEN: b2 = pos(x * q + y * p - x * y); break;
    case FR_BLEND_OVERLAY: b2 = 2 * y <= q ? 2 * x * y : light; break;
    case FR_BLEND_DARKEN: b2 = std::min(x * q, y * p); break;
    case FR_BLEND_LIGHTEN: b2 = std::max(x * q, y * p); break;
    case FR_BLEND_HARD_LIGHT: b2 = 2 * x <= p ? 2 * x * y : light; break;
    case FR_BLEND_DIFFERENCE: b2 = x * q > y * p ? x * q - y * p : y * p - x * q; break;
    case FR_BLEND_EXCLUSION: b2 = pos(x * q + y * p - 2 * x * y); break;
    }
    return x * (Q - q) + y * (Q - p) + b2;
}

uint32_t restated(uint32_t mode, int64_t Q, int64_t x, int64_t y, int64_t p, int64_t q)
{
    return (uint32_t)std::min(Q, (restated_n(mode, Q, x, y, p, q) + (Q - 1) / 2) / Q);
}

template <uint32_t MODE, uint32_t Q>
uint32_t shipped(uint32_t x, uint32_t y, uint32_t p, uint32_t q)
{
    return fr::blend_channel<MODE, Q>(x, y, p, q);
}

using Channel = uint32_t (*)(uint32_t, uint32_t, uint32_t, uint32_t);
template <uint32_t Q>
Channel channel_of(uint32_t mode)
{
    static const Channel k[FR_BLEND_PLUS] = {shipped<0, Q>, shipped<1, Q>, shipped<2, Q>, shipped<3, Q>, shipped<4, Q>, shipped<5, Q>, shipped<6, Q>, shipped<7, Q>};
    return k[mode];
}

// the sequence tests/test_layer_blend_ref.py draws again: Knuth's 64-bit LCG, the top 31 bits of each state
struct Lcg {
    uint64_t s;
    uint32_t next(uint32_t below)
    {
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        return (uint32_t)((s >> 33) % below);
    }
};

template <uint32_t Q>
void check_space()
{
    for (uint32_t mode = 0; mode < FR_BLEND_PLUS; ++mode) {
        const Channel f = channel_of<Q>(mode);
        const std::string name = fmt("px/%u/%s", Q, MODE_NAME[mode]);
        uint64_t corners = 0, random = 0, bad = 0, valid_over = 0;
        const auto one = [&](uint32_t x, uint32_t y, uint32_t p, uint32_t q) {
            if (f(x, y, p, q) != restated(mode, Q, x, y, p, q)) ++bad;
            if (x <= p && y <= q && restated_n(mode, Q, x, y, p, q) > (int64_t)Q * Q) ++valid_over;
        };
        const auto around = [](uint32_t top, uint32_t full) {   // 0, 1, top / 2 - 1 .. + 1, top - 1, top and the space's largest
            std::vector<uint32_t> v{0u, 1u, top / 2, top / 2 + 1, top, full};
            if (top / 2) v.push_back(top / 2 - 1);
            if (top) v.push_back(top - 1);
            for (uint32_t &e : v) e = std::min(e, full);
            return v;
        };
        for (uint32_t p : around(Q, Q))
            for (uint32_t q : around(Q, Q))
                for (uint32_t x : around(p, Q))
                    for (uint32_t y : around(q, Q)) one(x, y, p, q), ++corners;
        Lcg g{0x626c656e64ull + mode + 16u * Q};
        for (uint32_t i = 0; i < 2000000u; ++i, ++random) {
            const uint32_t p = g.next(Q + 1), q = g.next(Q + 1);
            // half the draws valid premultiplied, half any bytes
            const uint32_t x = g.next((i & 1u) ? Q + 1 : p + 1), y = g.next((i & 1u) ? Q + 1 : q + 1);
            one(x, y, p, q);
        }
        uint64_t digest = 0;
        Lcg d{12345u + mode};
        for (uint32_t i = 0; i < 4096u; ++i) {
            const uint32_t x = d.next(Q + 1), y = d.next(Q + 1), p = d.next(Q + 1), q = d.next(Q + 1);
            digest = digest * 31u + f(x, y, p, q);
        }
        printf("%s corners=%llu random=%llu bad=%llu valid_over=%llu digest=%llu\n", name.c_str(), (unsigned long long)corners, (unsigned long long)random,
               (unsigned long long)bad, (unsigned long long)valid_over, (unsigned long long)digest);
        require(bad == 0, name, "blend_channel differs from the 64-bit restatement");
        require(valid_over == 0, name, "N above Q^2 for a valid premultiplied input");
    }
}

void check_divisions()
{
    uint64_t bad = 0, n = 0;
    for (uint32_t v = 0; v < (1u << 24); ++v, ++n)
        if (fr::blend_div255(v) != v / 255u) ++bad;
    printf("div255 checked=%llu bad=%llu\n", (unsigned long long)n, (unsigned long long)bad);
    require(bad == 0, "div255", "blend_div255 is not n div 255 below 2^24");

    bad = n = 0;
    const auto three = [&](uint64_t k) {
        for (uint64_t v : {k * 65535u - (k ? 1u : 0u), k * 65535u, k * 65535u + 1u}) {
            if (v >= ((uint64_t)1 << 47)) continue;
            ++n;
            if (fr::blend_div65535(v) != v / 65535u) ++bad;
        }
    };
    const uint64_t top = 3ull * 65535u * 65535u + 65535u;       // above N + 32767 for any bytes
    for (uint64_t k = 0; k * 65535u <= top; ++k) three(k);
    const uint64_t last = (((uint64_t)1 << 47) - 1) / 65535u;   // the largest multiple in the stated range
    for (uint64_t i = 0; i <= (1u << 20); ++i) three(last - i * (last >> 20));
    three(last);
    printf("div65535 checked=%llu bad=%llu top=%llu\n", (unsigned long long)n, (unsigned long long)bad, (unsigned long long)top);
    require(bad == 0, "div65535", "blend_div65535 is not n div 65535");
}

void check_order()
{
    constexpr uintptr_t SRC = 0x10000000u, DST = 0x20000000u;
    const fr_layer_blit one[1] = {{0, 0, 10, 10, 0, 0, 255}}, loud[1] = {{0, 0, 10, 10, 0, 0, 256}};
    struct { const char *name; uintptr_t src; uint32_t flags, mode; const fr_layer_blit *blits; } C[] = {
        {"check/valid_plus", SRC, 0, FR_BLEND_PLUS, one},
        {"check/valid_srgb_multiply", SRC, FR_LAYER_SRGB, FR_BLEND_MULTIPLY, one},
        {"check/mode_9", SRC, 0, FR_BLEND_MODES, one},
        {"check/mode_max", SRC, 0, 0xffffffffu, one},
        {"check/flag_before_mode", SRC, FR_LCD_BGR, FR_BLEND_MODES, one},
        {"check/flag_mask_plane", SRC, FR_MASK_PLANE, 0, one},
        {"check/flag_mask_erase", SRC, FR_MASK_ERASE | FR_LAYER_SRGB, 0, one},
        {"check/mode_before_src", 0, 0, FR_BLEND_MODES, one},
        {"check/mode_before_opacity", SRC, 0, FR_BLEND_MODES, loud},
        {"check/src_null", 0, 0, 0, one},
        {"check/opacity_256", SRC, 0, 0, loud},
    };
    for (const auto &c : C) {
        const fr::LayerIn in{c.src, DST, 300, 50, 132, 50, c.blits, 1, c.flags};
        fr::LayerTables t, plain;
        clear_error();
        const int rc = fr::layer_blend_tables(in, c.mode, t);
        if (rc) {
            printf("%s rc=%d | err=%s\n", c.name, rc, last_error());
            continue;
        }
        printf("%s rc=0 | tiles=%zu\n", c.name, t.tiles.size());
        // an accepted call's tables are fr_layer_over's
        const int rc2 = fr::layer_tables(in, plain);
        bool same = rc2 == 0 && plain.tiles.size() == t.tiles.size() && plain.opacity == t.opacity;
        for (size_t i = 0; same && i < t.tiles.size(); ++i) {
            const fr::LayerTile &a = t.tiles[i], &b = plain.tiles[i];
            same = a.x == b.x && a.y == b.y && a.x0 == b.x0 && a.x1 == b.x1 && a.y1 == b.y1 && a.sx == b.sx && a.sy == b.sy && a.ov == b.ov;
        }
        require(same, c.name, "the tables differ from layer_tables'");
    }
}

}  // namespace

int main()
{
    check_divisions();
    check_space<255u>();
    check_space<65535u>();
    check_order();
    return exit_status();
}

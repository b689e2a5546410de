// fr_layer_blend_math.hpp — the arithmetic of fr_layer_blend for one colour byte (include/fr_raster.h; DESIGN.md sections
// 4.16 and 5), and the order of the call's checks.  Plain C++ that also compiles as HIP: blend_px (fr_layer_px.hpp) calls
// blend_channel on the device, and host/layer_blend_selftest.cpp checks the same text on the CPU against a restatement in
// 64-bit integers and the two divisions over their whole stated ranges.
#pragma once
#include "fr_layer_plan.hpp"

#include <cstdint>
#include <type_traits>

#if defined(__HIP__) || defined(__HIPCC__)
#define FR_BLEND_FN __host__ __device__ __forceinline__
#else
#define FR_BLEND_FN inline
#endif

namespace fr {

// n div 255 for n < 2^24 (exact over that whole range: the self-test checks every n).  N + 127 of the UNORM definition is
// below 3 * 255^2 + 128 < 2^18.  On the device a 24 x 24-bit product (v_mul_hi_u32_u24).
FR_BLEND_FN uint32_t blend_div255(uint32_t n)
{
    return (uint32_t)(((uint64_t)(n & 0xffffffu) * 0x808081u) >> 31);
}

// n div 65535 for n < 2^47, by folding: no multiply.  65536 = 65535 + 1, so with h = n >> 16 and l = n & 0xffff,
// n = 65535 h + t where t = h + l < 2^31 + 2^16; once more, t = 65535 (t >> 16) + u with u = (t >> 16) + (t & 0xffff).
// t >> 16 <= 2^15, so u < 2^15 + 2^16 < 2 * 65535, and n = 65535 (h + (t >> 16)) + u with 0 <= u < 2 * 65535:
// n div 65535 = h + (t >> 16) + (u >= 65535).  N + 32767 of the linear-light definition is below 3 * 65535^2 + 32768
// < 2^34, for which h < 2^18 and everything after the first shift is 32-bit arithmetic.
FR_BLEND_FN uint64_t blend_div65535(uint64_t n)
{
    const uint64_t h = n >> 16;
    const uint32_t t = (uint32_t)h + ((uint32_t)n & 0xffffu);
    const uint32_t u = (t >> 16) + (t & 0xffffu);
    return h + (t >> 16) + (u >= 65535u ? 1u : 0u);
}

// a - b where that is positive, else 0
FR_BLEND_FN uint32_t blend_pos(uint32_t a, uint32_t b) { return a > b ? a - b : 0u; }

// One colour byte of fr_layer_blend for the modes that go through N: `out` of the header for a layer value x under its
// alpha p and a destination value y under its alpha q, all four in [0, Q], Q = 255 or 65535.  Every product has two factors
// of at most 16 bits, so it fits 32 bits (a 24-bit multiply on the device wherever the compiler sees the range: DESIGN.md
// section 4.16); only sums of products are kept in 64 bits (N can reach 3 Q^2, above 2^32 for Q = 65535), and the source
// asks for no 64-bit multiply.
template <uint32_t MODE, uint32_t Q>
FR_BLEND_FN uint32_t blend_channel(uint32_t x, uint32_t y, uint32_t p, uint32_t q)
{
    static_assert(Q == 255u || Q == 65535u, "UNORM or linear light");
    static_assert(MODE < FR_BLEND_PLUS, "PLUS has no N");
    using U = std::conditional_t<Q == 255u, uint32_t, uint64_t>;   // N <= 3 Q^2 fits 32 bits for Q = 255
    using S = std::conditional_t<Q == 255u, int32_t, int64_t>;
    const uint32_t xq = x * q, yp = y * p, xy = x * y;
    // 2 x y where the side that decides is dark, p q - 2 (q - y)+ (p - x)+ where it is light
    const auto light = [&]() -> U {
        const S v = (S)(p * q) - 2 * (S)(blend_pos(q, y) * blend_pos(p, x));
        return v > 0 ? (U)v : 0u;
    };
    U b2 = 0;
    if constexpr (MODE == FR_BLEND_MULTIPLY) b2 = xy;
    else if constexpr (MODE == FR_BLEND_SCREEN) {
        const S v = (S)xq + (S)yp - (S)xy;
        b2 = v > 0 ? (U)v : 0u;
    } else if constexpr (MODE == FR_BLEND_DARKEN) b2 = xq < yp ? xq : yp;
    else if constexpr (MODE == FR_BLEND_LIGHTEN) b2 = xq > yp ? xq : yp;
    else if constexpr (MODE == FR_BLEND_DIFFERENCE) b2 = xq > yp ? xq - yp : yp - xq;
    else if constexpr (MODE == FR_BLEND_EXCLUSION) {
        const S v = (S)xq + (S)yp - 2 * (S)xy;
        b2 = v > 0 ? (U)v : 0u;
    } else if constexpr (MODE == FR_BLEND_HARD_LIGHT) b2 = 2u * x <= p ? 2 * (U)xy : light();
    else b2 = 2u * y <= q ? 2 * (U)xy : light();        // FR_BLEND_OVERLAY
    const U n = (U)(x * (Q - q)) + (U)(y * (Q - p)) + b2 + (Q - 1u) / 2u;
    uint32_t out;
    if constexpr (Q == 255u) out = blend_div255((uint32_t)n);
    else out = (uint32_t)blend_div65535(n);
    return out < Q ? out : Q;
}

// The checks of fr_layer_blend in the header's order: fr_layer_over's, with the mode straight after the flag bits.
inline int layer_blend_tables(const LayerIn &in, uint32_t mode, LayerTables &out)
{
    out = LayerTables{};
    if (in.flags & ~(uint32_t)FR_LAYER_SRGB) return set_error(FR_E_INVALID, "unknown flag bits 0x%x", in.flags & ~(uint32_t)FR_LAYER_SRGB);
    if (mode >= FR_BLEND_MODES) return set_error(FR_E_INVALID, "blend mode %u: expected 0 .. %u", mode, FR_BLEND_MODES - 1u);
    return layer_tables(in, out);
}

}  // namespace fr

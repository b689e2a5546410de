// fr_text_colour.hpp — what the two translation units of text kernels (fr_text.hip, fr_text_affine.hip) both need around
// the row bodies they include: the colour arithmetic of fr_text_colour_kernel.inc, the FR_TEXT_LOAD_SKIP default and
// dependent_t.
#pragma once
#include <cstdint>
#include <type_traits>

namespace fr {

// Two 8-bit channels at once, in bits 0-7 and 16-23 of a word: (x + 127) div 255 with x = C*A + c*(255 - A) in [0, 65025]
// as (t + (t >> 8)) >> 8, t = x + 128 (exact over that whole domain: tests/test_text_rgba_ref.py checks every x).
// t + (t >> 8) < 2^16, so the halves never carry into each other.  c2: the sample's two channels; cA2 = C2 * A + 128 each.
__device__ __forceinline__ uint32_t blend2(uint32_t c2, uint32_t cA2, uint32_t ia)
{
    const uint32_t t = c2 * ia + cA2;
    return ((t + ((t >> 8) & 0x00ff00ffu)) >> 8) & 0x00ff00ffu;
}

// E(L), L in [0, 65535], from the LDS copy of SRGB_K: one lookup and one compare (fr_srgb.hpp)
__device__ __forceinline__ uint32_t srgb_encode(const uint16_t *K, uint32_t L)
{
    const uint32_t k = K[L >> 4];
    return (k & 0xffu) + ((L & 15u) >= (k >> 8) ? 1u : 0u);
}

// (x + 127) div 255 for x = D[C] * A + D[c] * (255 - A) <= 65535 * 255, given y = x + 127 < 2^24: (y * 0x808081) >> 31,
// a 24 x 24-bit product (v_mul_u32_u24, v_mul_hi_u32_u24; exact over that whole domain: tests/test_text_srgb_ref.py
// checks every y)
__device__ __forceinline__ uint32_t div255_24(uint32_t y)
{
    return (uint32_t)(((uint64_t)(y & 0xffffffu) * 0x808081u) >> 31);
}

// FR_TEXT_LOAD_SKIP=0 (an experiment build only: make variant) makes the LOAD kernels, those of both placement forms,
// store every pixel, to price the store skip of the colour body (fr_text.hip).
#ifndef FR_TEXT_LOAD_SKIP
#define FR_TEXT_LOAD_SKIP 1
#endif

// T, as a type that depends on N: a body included straight into a kernel template names members of the other placement
// form's instance under if constexpr (PLACE), which only a dependent type leaves unchecked in the discarded branch
template <int N, class T>
using dependent_t = std::conditional_t<(N > 0), T, void>;

}  // namespace fr

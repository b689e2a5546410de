// fr_layer_tint.hpp — what the kernels that write a tinted layer share (fr_layer_shadow.hip, fr_layer_outline.hip): the
// stored element of one alpha under a straight colour, and the store of four such elements of one row.
#pragma once
#include "fr_srgb.hpp"
#include "fr_text_colour.hpp"

namespace fr {

// the stored element for one alpha: (m(R, a), m(G, a), m(B, a), a) or its sRGB form, a = m(alpha, A)
__device__ __forceinline__ uint32_t tint_of(uint32_t alpha, uint32_t rgba, uint32_t srgb)
{
    constexpr uint32_t M2 = 0x00ff00ffu, HALF2 = 0x00800080u;
    const uint32_t a = blend2(alpha, HALF2, rgba >> 24) & 0xffu;
    if (!srgb) return blend2(rgba & M2, HALF2, a) | blend2((rgba >> 8) & 0xffu, HALF2, a) << 8 | a << 24;
    uint32_t out = a << 24;
#pragma unroll
    for (int c = 0; c < 3; ++c) out |= srgb_encode(SRGB_K, div255_24((uint32_t)SRGB_D[(rgba >> (8 * c)) & 0xffu] * a + 127u)) << (8 * c);
    return out;
}

// Four pixels of one row from p on, their alphas in the bytes of `al`, tinted through `lut` (tint_of of every alpha): one
// 16-byte store where all four are inside the rectangle (valid == 15) and `vec` says that p sits on the 16-byte grid,
// else pixel by pixel and only where `valid` has the pixel's bit.
__device__ __forceinline__ void store_tinted4(uint32_t *p, uint32_t al, uint32_t valid, uint32_t vec, const uint32_t *lut)
{
    if (valid == 15u && vec) {
        *reinterpret_cast<uint4 *>(p) = make_uint4(lut[al & 0xffu], lut[(al >> 8) & 0xffu], lut[(al >> 16) & 0xffu], lut[al >> 24]);
    } else {
#pragma unroll
        for (uint32_t i = 0; i < 4u; ++i)
            if (valid >> i & 1u) p[i] = lut[(al >> (8u * i)) & 0xffu];
    }
}

}  // namespace fr

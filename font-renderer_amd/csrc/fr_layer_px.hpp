// fr_layer_px.hpp — source-over of one premultiplied pixel, for the kernels that composite onto an image: layer_over_kernel
// (fr_layer.hip), layer_rects_kernel (fr_layer_rects.hip), layer_paint_kernel (fr_layer_paint.hip) and layer_mask_kernel
// (fr_layer_mask.hip) with its erase, layer_warp_kernel (fr_layer_warp.hip) with its linear-light sibling, and its variant with one alpha per colour byte for layer_lcd_kernel
// (fr_layer_lcd.hip).  The arithmetic is that of the text plans' colour body (fr_text_colour.hpp), per pixel instead of per
// sample.  blend_px, the pixel of layer_blend_kernel (fr_layer_blend.hip), takes its colour bytes through blend_channel
// (fr_layer_blend_math.hpp), which the host compiles too.
#pragma once
#include "fr_layer_blend_math.hpp"
#include "fr_text_colour.hpp"

namespace fr {

inline constexpr uint32_t M2 = 0x00ff00ffu, HALF2 = 0x00800080u;

// m(x, y) = (x * y + 127) div 255 on the two channels of c2 at once: blend2 with a colour term of zero
__device__ __forceinline__ uint32_t m2(uint32_t c2, uint32_t y) { return blend2(c2, HALF2, y); }

// the two 16-bit halves of v, each at most 510, clamped to 255
__device__ __forceinline__ uint32_t clamp2(uint32_t v)
{
    return min(v & 0xffffu, 255u) | (min(v >> 16, 255u) << 16);
}

// a' = m(s_a, o) of the layer pixel s
template <int OPACITY>
__device__ __forceinline__ uint32_t alpha_of(uint32_t s, uint32_t o)
{
    return OPACITY ? m2(s >> 24, o) : s >> 24;
}

// The definition of fr_layer_over for one pixel: s over d at opacity o.  s == 0 gives d (consequence 1), and with
// a' == 255 no bit of d reaches the result, so the caller may pass anything for a destination it did not load.
template <int SRGB, int OPACITY>
__device__ __forceinline__ uint32_t over_px(uint32_t s, uint32_t d, uint32_t o, const uint16_t *D, const uint16_t *K)
{
    uint32_t s1a = (s >> 8) & M2;                              // channel 1 and alpha
    if (OPACITY) s1a = m2(s1a, o);
    const uint32_t ia = 255u - (s1a >> 16);
    const uint32_t r1a = s1a + m2((d >> 8) & M2, ia);          // alpha: a' + m(d_a, 255 - a') <= 255
    if constexpr (!SRGB) {
        uint32_t s02 = s & M2;
        if (OPACITY) s02 = m2(s02, o);
        return clamp2(s02 + m2(d & M2, ia)) | (clamp2(r1a) << 8);
    } else {
        uint32_t out = 0u;                                     // a shift register: a channel enters at the top byte
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            uint32_t S = D[(s >> (8 * c)) & 0xffu];
            if (OPACITY) S = div255_24(S * o + 127u);
            const uint32_t L = min(65535u, S + div255_24((uint32_t)D[(d >> (8 * c)) & 0xffu] * ia + 127u));
            out = (out >> 8) | (srgb_encode(K, L) << 24);
        }
        return (out >> 8) | (r1a & 0x00ff0000u) << 8;          // alpha is stored linearly
    }
}

// The definition of fr_layer_blend for one pixel: s blended into d in mode MODE at opacity o.  s == 0 gives d in every mode
// (consequence 2: x = p = 0 leaves N = y Q, and E(D[v]) = v); unlike over_px it needs d whatever the layer's alpha is.
template <int SRGB, uint32_t MODE, int OPACITY>
__device__ __forceinline__ uint32_t blend_px(uint32_t s, uint32_t d, uint32_t o, const uint16_t *D, const uint16_t *K)
{
    constexpr bool PLUS = MODE == FR_BLEND_PLUS;
    uint32_t s1a = (s >> 8) & M2;                              // channel 1 and alpha
    if (OPACITY) s1a = m2(s1a, o);
    const uint32_t a1 = s1a >> 16, da = d >> 24;
    const uint32_t out_a = PLUS ? min(255u, a1 + da) : a1 + m2(da, 255u - a1);     // a' + m(d_a, 255 - a') <= 255
    if constexpr (!SRGB) {
        uint32_t s02 = s & M2;
        if (OPACITY) s02 = m2(s02, o);
        const uint32_t x[3] = {s02 & 0xffu, s1a & 0xffu, s02 >> 16};
        uint32_t out = out_a << 24;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const uint32_t y = (d >> (8 * c)) & 0xffu;
            uint32_t v;
            if constexpr (PLUS) v = min(255u, x[c] + y);
            else v = blend_channel<MODE, 255u>(x[c], y, a1, da);
            out |= v << (8 * c);
        }
        return out;
    } else {
        [[maybe_unused]] const uint32_t p = 257u * a1, q = 257u * da;
        uint32_t out = 0u;                                     // a shift register: a channel enters at the top byte
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            uint32_t X = D[(s >> (8 * c)) & 0xffu];
            if (OPACITY) X = div255_24(X * o + 127u);
            const uint32_t Y = D[(d >> (8 * c)) & 0xffu];
            uint32_t L;
            if constexpr (PLUS) L = min(65535u, X + Y);
            else L = blend_channel<MODE, 65535u>(X, Y, p, q);
            out = (out >> 8) | (srgb_encode(K, L) << 24);
        }
        return (out >> 8) | out_a << 24;                       // alpha is stored linearly
    }
}

// over_px in linear light for a layer pixel that comes as linear values: the definition of fr_layer_warp with FR_LAYER_SRGB,
// where the sampler hands over S[c], 16 bits each, in the place of D[s_c], and the sampled alpha sa.  sa == 0 with S == 0
// gives d, and with a' == 255 no bit of d reaches the result, as for over_px.
template <int OPACITY>
__device__ __forceinline__ uint32_t over_px_lin(uint32_t sa, const uint32_t (&S)[3], uint32_t d, uint32_t o, const uint16_t *D, const uint16_t *K)
{
    const uint32_t a1 = OPACITY ? m2(sa, o) : sa;
    const uint32_t ia = 255u - a1;
    uint32_t out = 0u;                                         // a shift register: a channel enters at the top byte
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        uint32_t Sc = S[c];
        if (OPACITY) Sc = div255_24(Sc * o + 127u);
        const uint32_t L = min(65535u, Sc + div255_24((uint32_t)D[(d >> (8 * c)) & 0xffu] * ia + 127u));
        out = (out >> 8) | (srgb_encode(K, L) << 24);
    }
    return (out >> 8) | (a1 + m2(d >> 24, ia)) << 24;          // alpha is stored linearly; a' + m(d_a, 255 - a') <= 255
}

// The erase of fr_layer_mask for one pixel: d times 255 - t (destination-out).  t == 0 gives d (m(x, 255) = x, E(D[v]) = v)
// and t == 255 gives 0 whatever d is, so the caller may pass anything for a destination it did not load.
template <int SRGB>
__device__ __forceinline__ uint32_t erase_px(uint32_t d, uint32_t t, const uint16_t *D, const uint16_t *K)
{
    const uint32_t ia = 255u - t;
    const uint32_t r1a = m2((d >> 8) & M2, ia);                // channel 1 and alpha
    if constexpr (!SRGB) {
        return m2(d & M2, ia) | r1a << 8;
    } else {
        uint32_t out = 0u;                                     // a shift register: a channel enters at the top byte
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const uint32_t L = div255_24((uint32_t)D[(d >> (8 * c)) & 0xffu] * ia + 127u);
            out = (out >> 8) | (srgb_encode(K, L) << 24);
        }
        return (out >> 8) | (r1a & 0x00ff0000u) << 8;          // alpha is stored linearly
    }
}

// The definition of fr_layer_lcd for one pixel, component alpha: colour byte b of the straight colour over d through an
// alpha al[b] of its own; the pixel's alpha through the largest of the three.  cl[b]: the colour's byte b, or D of it in
// linear light.  al = (0, 0, 0) gives d (E(D[v]) = v), and with al = (255, 255, 255) no bit of d reaches the result.
template <int SRGB>
__device__ __forceinline__ uint32_t over_px_ca(const uint32_t (&cl)[3], uint32_t d, const uint32_t (&al)[3], const uint16_t *D, const uint16_t *K)
{
    const uint32_t amax = max(al[0], max(al[1], al[2]));
    uint32_t out = (amax + m2(d >> 24, 255u - amax)) << 24;    // a_max + m(d_a, 255 - a_max) <= 255
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const uint32_t dc = (d >> (8 * c)) & 0xffu, ia = 255u - al[c];
        if constexpr (!SRGB) {
            out |= min(255u, m2(cl[c], al[c]) + m2(dc, ia)) << (8 * c);
        } else {
            const uint32_t L = min(65535u, div255_24(cl[c] * al[c] + 127u) + div255_24((uint32_t)D[dc] * ia + 127u));
            out |= srgb_encode(K, L) << (8 * c);
        }
    }
    return out;
}

}  // namespace fr

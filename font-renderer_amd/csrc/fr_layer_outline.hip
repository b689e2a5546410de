// fr_layer_outline.hip — the kernel of fr_layer_outline (include/fr_raster.h; DESIGN.md sections 4.13 and 5): the maximum of
// a layer's alpha (or of its complement) weighted by a disc, combined with the layer's own alpha by the kind and tinted
// into the destination.  Per kernel row the weight is 255 on a core and below it on a few rim offsets: the core is a range
// maximum read from running-maximum levels, only the rim is multiplied.  The host side (fr_layer_outline_plan.cpp) makes
// the weights, says which levels are needed and which tiles can hold anything.
#include "fr_layer_outline.hpp"
#include "fr_layer_tint.hpp"

namespace fr {

namespace {

constexpr uint32_t M2 = 0x00ff00ffu, HALF2 = 0x00800080u;
constexpr uint32_t T = SHADOW_TILE, THREADS = 256;

typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));

// the maximum of each 16-bit half (v_pk_max_u16)
__device__ __forceinline__ uint32_t max2(uint32_t a, uint32_t b)
{
    return __builtin_bit_cast(uint32_t, __builtin_elementwise_max(__builtin_bit_cast(u16x2, a), __builtin_bit_cast(u16x2, b)));
}

// the four bytes from byte c of the row p on, c + 3 inside the row's words but for the last
__device__ __forceinline__ uint32_t fetch4(const uint32_t *p, uint32_t c) { return __builtin_amdgcn_alignbyte(p[(c >> 2) + 1u], p[c >> 2], c & 3u); }

__device__ __forceinline__ int32_t clamp_to(int64_t v, int32_t hi) { return (int32_t)(v < 0 ? 0 : v > hi ? hi : v); }

}  // namespace

// One workgroup of 256 threads makes one 64 x 64 tile of the rectangle, as layer_shadow_kernel does; blockIdx.x counts the
// tiles row by row, and the tile columns start a.lead pixels left of the rectangle.
//   0. Every thread makes one entry of the tint of all 256 alphas in LDS, and the table comes into LDS too: read from global
//      memory inside the loops, its words cost a vector load and a full wait each.  A tile that a.live does not touch stores
//      the tint of 0 and is done.
//   1. The tile's alpha and a halo of R rows and R4 columns (R rounded up to whole words) go into LDS as bytes, rows of
//      outline_lds_words(R) words: wave w takes rows w, w + 4, ..; a pixel outside the window is 0 and not loaded.  COMPLEMENT
//      stores 255 - alpha, which is 255 outside the window.  This is level 0.
//   2. Levels.  Byte c of a row of level l + 1 is the maximum of bytes c and c + 2^l of level l, so the maximum of the 2^(l + 1)
//      bytes from c on (fewer at the row's end, where no window reaches).  Half a wave takes a row, a word per lane, the two
//      byte pairs of a word by v_pk_max_u16; a.levels levels, as many as the widest core needs.
//   3. Thread (row r, group g of four pixels) of each quarter of the tile walks the kernel rows j.  Core: the range of
//      2 core + 1 bytes around each of its pixels is covered by two windows of 2^k bytes, k = floor(log2(2 core + 1)), so the
//      four pixels' range maxima are two unaligned words of level k, each cut from two whole words (v_alignbyte_b32); they go
//      into maxima that are multiplied by 255 once, at the end.  Rim: for each of the row's `rim` offsets the two unaligned
//      words of level 0 at -i and +i (K is even in i), their maximum multiplied by the weight as two 16-bit halves (255 * 255
//      fits), kept as running maxima of the raw products for pixels 0 and 2 and pixels 1 and 3.  The row record sits in
//      scalar registers; the weight is an LDS broadcast.
//   4. One (x + 127) div 255 per pixel, on two halves at once, gives G; the kind's alpha follows from G and the tile's own
//      byte: G, G - A0, A0 - (255 - G) or 255 - G, all four pixels in one word (no byte borrows: G >= A and S <= A0).
//   5. Out, as layer_shadow_kernel's tint: one 16-byte store or single pixels (store_tinted4).
// POST: the kind subtracts (RING, INNER).
template <int COMPLEMENT, int POST>
__global__ __launch_bounds__(THREADS) void layer_outline_kernel(OutlineArgs a)
{
    extern __shared__ uint4 lds_raw[];
    __shared__ uint32_t lut[256];
    __shared__ uint4 tab[OUTLINE_MAX_UNITS];
    const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
    const uint32_t R = a.reach, R4 = (R + 3u) & ~3u, PW = outline_lds_words(R), LH = T + 2u * R, LW = 4u * PW;
    uint32_t *const inw = reinterpret_cast<uint32_t *>(lds_raw);
    uint8_t *const in = reinterpret_cast<uint8_t *>(lds_raw);

    lut[t] = tint_of(t, a.rgba, a.srgb);
    for (uint32_t i = t; i < a.units; i += THREADS) tab[i] = a.table[i];

    const uint32_t tile_x = blockIdx.x % a.tiles_x, tile_y = blockIdx.x / a.tiles_x;
    // the tile in the rectangle's coordinates against a.live
    const int64_t tx0 = (int64_t)tile_x * T - a.lead, ty0 = (int64_t)tile_y * T;
    const bool live = tx0 < (int64_t)a.live_x1 && tx0 + T > (int64_t)a.live_x0 && ty0 < (int64_t)a.live_y1 && ty0 + T > (int64_t)a.live_y0;
    // ---- 1. the input tile
    if (live) {
        const int64_t bx = tx0 + a.off_x - R4, by = ty0 + a.off_y - R;
        const uint32_t c0 = clamp_to(-bx, LW), c1 = clamp_to((int64_t)a.in_w - bx, LW);
        const uint32_t r0 = clamp_to(-by, LH), r1 = clamp_to((int64_t)a.in_h - by, LH);
        for (uint32_t r = wave; r < LH; r += THREADS / 64) {
            const bool row_in = r >= r0 && r < r1;
            const uint64_t row_at = row_in ? (uint64_t)(by + r) * a.in_pitch : 0u;
            for (uint32_t c = lane; c < LW; c += 64) {
                uint32_t v = 0u;
                if (row_in && c >= c0 && c < c1) v = a.in[row_at + (uint64_t)(bx + c)] >> 24;
                in[r * LW + c] = (uint8_t)(COMPLEMENT ? 255u - v : v);
            }
        }
    }
    __syncthreads();
    // ---- 2. the levels
    const uint32_t LV = LH * PW;                                // words of a level
    if (live) {
        for (uint32_t l = 0; l < a.levels; ++l) {
            const uint32_t sh = 1u << l, q = t & 31u;
            for (uint32_t r = t >> 5; r < LH && q < PW; r += THREADS / 32) {
                const uint32_t *const src = inw + l * LV + r * PW;
                const uint32_t x = src[q];
                uint32_t y;                                     // the bytes 2^l further on; beyond the row's end: none
                if (sh < 4u) y = __builtin_amdgcn_alignbyte(q + 1u < PW ? src[q + 1u] : 0u, x, sh);
                else y = q + (sh >> 2) < PW ? src[q + (sh >> 2)] : 0u;
                inw[(l + 1u) * LV + r * PW + q] = max2(x & M2, y & M2) | max2((x >> 8) & M2, (y >> 8) & M2) << 8;
            }
            __syncthreads();
        }
    }

    const uint32_t g = t & 15u;
    const int64_t X0 = tx0 + 4u * g;                           // the rectangle's column of the group's first pixel
    uint32_t valid = 0u;
#pragma unroll
    for (uint32_t i = 0; i < 4u; ++i) valid |= (X0 + i >= 0 && X0 + i < (int64_t)a.out_w) ? 1u << i : 0u;
    if (!valid) return;
    const uint8_t *const weights = reinterpret_cast<const uint8_t *>(tab + (2u * R + 1u));   // tap i + R4 of row jj at [jj * 4 NW + R4 + i]
    const uint32_t NW = R4 / 2u + 1u;
#pragma unroll 1
    for (uint32_t it = 0; it < 4u; ++it) {
        const uint32_t row = 16u * it + (t >> 4), y = tile_y * T + row;
        if (y >= a.out_h) continue;
        uint32_t al = 0u;
        if (live) {
            // ---- 3. the maxima of the raw products, and of the cores (not yet multiplied by 255): pixels 0 and 2, pixels 1 and 3
            uint32_t acc02 = 0u, acc13 = 0u, c02 = 0u, c13 = 0u;
            for (uint32_t jj = 0; jj <= 2u * R; ++jj) {
                const int32_t core = (int32_t)__builtin_amdgcn_readfirstlane(tab[jj].x);
                const uint32_t rim = __builtin_amdgcn_readfirstlane(tab[jj].y), k = __builtin_amdgcn_readfirstlane(tab[jj].z);
                const uint32_t *const p = inw + (row + jj) * PW + g;
                if (core >= 0) {
                    const uint32_t w1 = fetch4(p + k * LV, R4 - core), w2 = fetch4(p + k * LV, R4 + core + 1u - (1u << k));
                    c02 = max2(c02, max2(w1 & M2, w2 & M2));
                    c13 = max2(c13, max2((w1 >> 8) & M2, (w2 >> 8) & M2));
                }
                for (uint32_t n = 0; n < rim; ++n) {
                    const uint32_t i = (uint32_t)(core + 1) + n, kw = weights[jj * NW * 4u + R4 + i];
                    const uint32_t w1 = fetch4(p, R4 - i), w2 = fetch4(p, R4 + i);
                    acc02 = max2(acc02, max2(w1 & M2, w2 & M2) * kw);
                    acc13 = max2(acc13, max2((w1 >> 8) & M2, (w2 >> 8) & M2) * kw);
                }
            }
            acc02 = max2(acc02, c02 * 255u);
            acc13 = max2(acc13, c13 * 255u);
            // ---- 4. G = (x + 127) div 255 as (t + (t >> 8)) >> 8, t = x + 128 (blend2's form; t + (t >> 8) stays below 2^16)
            const uint32_t t02 = acc02 + HALF2, t13 = acc13 + HALF2;
            const uint32_t G = (((t02 + ((t02 >> 8) & M2)) >> 8) & M2) | ((t13 + ((t13 >> 8) & M2)) & 0xff00ff00u);
            const uint32_t own = inw[(row + R) * PW + g + R4 / 4u];      // the group's own bytes (complemented with COMPLEMENT)
            if constexpr (!COMPLEMENT) al = POST ? G - own : G;
            else al = POST ? ~own - ~G : ~G;
        }
        // ---- 5. out
        store_tinted4(a.out + ((int64_t)((uint64_t)y * a.out_pitch) + X0), al, valid, a.vec, lut);
    }
}

hipError_t launch_layer_outline(uint32_t kind, uint32_t tiles, const OutlineArgs &a, hipStream_t stream)
{
    using Kern = void (*)(OutlineArgs);
    static const Kern kern[4] = {layer_outline_kernel<0, 0>, layer_outline_kernel<0, 1>, layer_outline_kernel<1, 1>, layer_outline_kernel<1, 0>};
    if (kind > FR_OUTLINE_SHRINK || a.reach > OUTLINE_MAX_REACH || a.units > OUTLINE_MAX_UNITS || a.levels > OUTLINE_MAX_LEVELS || !a.tiles_x || tiles % a.tiles_x || tiles > SHADOW_MAX_TILES) return hipErrorInvalidValue;
    hipLaunchKernelGGL(kern[kind], dim3(tiles), dim3(THREADS), outline_lds_bytes(a.reach, a.levels), stream, a);
    return hipGetLastError();
}

}  // namespace fr

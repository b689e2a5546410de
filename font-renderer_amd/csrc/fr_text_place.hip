// fr_text_place.hip — text runs of fr_glyph_place_ex placements (include/fr_raster.h, DESIGN.md sections 4.7 and 5):
// every instance has its own scale, a slant and a baseline kept to 1/64 pixel.  The work layout, tables, records, colour
// arithmetic and stores are those of fr_text.hip (one workgroup of four waves per 64 x 16 tile, a wave per row, a pixel
// per lane, the instance list of the tile walked per row); only the map from a sample to the glyph's font units differs:
//     cy = (f32(iy - Y) + (fy - off(j))) / s,   t = (f32(X - ix) + (off(i) - fx)) / s,   cx = t - k * cy
// For one row and one instance cy, s, k and k * cy are still the same in all lanes, so a record's root is evaluated once
// per wave, as in text_kernel; the slant costs the lanes n subtracts per accepted root
// (fr_text_place_mask_kernel.inc).  fr_text.hip is not touched: plans of fr_glyph_place placements launch its kernels.
//
// text_place_kernel: coverage / mask bytes.  text_place_rgba_kernel, text_place_srgb_kernel and their _load_ forms: RGBA
// pixels, one body (place_colour_rows) whose SRGB / LOAD parameters select what text_rgba_kernel, text_srgb_kernel,
// text_rgba_load_kernel and text_srgb_load_kernel do.  KEEP IN STEP with those four: the walk, blend and resolve here
// are theirs, and so are blend2, srgb_encode and div255_24 below (copies, so that fr_text.hip's object code cannot move).
#include "fr_text.hpp"
#include "fr_srgb.hpp"

#include <cstdio>

namespace fr {
namespace {

// == fr_text.hip's blend2: two 8-bit channels at once, (x + 127) div 255 for x = C*A + c*(255 - A)
__device__ __forceinline__ uint32_t place_blend2(uint32_t c2, uint32_t cA2, uint32_t ia)
{
    const uint32_t t = c2 * ia + cA2;
    return ((t + ((t >> 8) & 0x00ff00ffu)) >> 8) & 0x00ff00ffu;
}

// == fr_text.hip's srgb_encode: E(L), L in [0, 65535], from the LDS copy of SRGB_K
__device__ __forceinline__ uint32_t place_srgb_encode(const uint16_t *K, uint32_t L)
{
    const uint32_t k = K[L >> 4];
    return (k & 0xffu) + ((L & 15u) >= (k >> 8) ? 1u : 0u);
}

// == fr_text.hip's div255_24: (x + 127) div 255 given y = x + 127 < 2^24
__device__ __forceinline__ uint32_t place_div255_24(uint32_t y)
{
    return (uint32_t)(((uint64_t)(y & 0xffffffu) * 0x808081u) >> 31);
}

}  // namespace

template <int N, int FILL>
__global__ __launch_bounds__(64 * TEXT_WAVES) void text_place_kernel(TextPlaceArgs a)
{
    const TextTile tl = a.tiles[blockIdx.x];
    const TextRun rn = a.runs[tl.run];
    const int lane = (int)(threadIdx.x & 63u);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int X = (int)tl.x0 + lane;
    float off[N];
#pragma unroll
    for (int k = 0; k < N; ++k) off[k] = sub_off(k, N, a.phase_center);
    for (int yy = wave; yy < TEXT_TILE_H; yy += TEXT_WAVES) {
        const int Y = (int)tl.y0 + yy;
        if (Y >= (int)rn.h) break;
        uint32_t mask = 0u;
        for (uint32_t q = tl.lbeg; q < tl.lend; ++q) {
            const TextInstEx in = a.insts[a.list[q]];
            if (Y < in.y0 || Y >= in.y1) continue;                       // (wave-uniform)
            const bool inside = X >= in.x0 && X < in.x1;
#include "fr_text_place_mask_kernel.inc"
            if (inside) mask |= m;
        }
        if (X < (int)rn.w) {
            constexpr uint32_t NN = (uint32_t)(N * N);
            const uint8_t v = (uint8_t)((510u * (uint32_t)__builtin_popcount(mask) + NN) / (2u * NN));    // round_half_up(255 k / n^2)
            uint8_t *dst = a.out + ((uint64_t)rn.out_y + (uint64_t)Y) * a.out_stride + rn.out_x + (uint32_t)X;
            __builtin_nontemporal_store(v, dst);
        }
    }
}

// The rows of one tile for the four RGBA families.  SRGB: blend and resolve in 16-bit linear light through D and K (the
// LDS copies of SRGB_D / SRGB_K; unused otherwise).  LOAD: every sample starts at the pixel in the output instead of the
// run's clear colour, and a lane whose samples are all untaken (BLEND = 0) skips its store.  BLEND = 0: the instances are
// walked backwards and each adds the samples it takes first; BLEND = 1: n^2 sample states per lane, blended forwards.
template <int N, int FILL, int BLEND, bool SRGB, bool LOAD>
__device__ __forceinline__ void place_colour_rows(const TextPlaceArgs &a, const uint16_t *D, const uint16_t *K)
{
    constexpr uint32_t NN = (uint32_t)(N * N);
    constexpr uint32_t FULL = NN == 32u ? ~0u : (1u << NN) - 1u;
    constexpr uint32_t LG = N == 4 ? 4u : N == 2 ? 2u : 0u;              // log2(n^2)
    constexpr uint32_t M2 = 0x00ff00ffu;
    const TextTile tl = a.tiles[blockIdx.x];
    const TextRun rn = a.runs[tl.run];
    const int lane = (int)(threadIdx.x & 63u);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int X = (int)tl.x0 + lane;
    float off[N];
#pragma unroll
    for (int k = 0; k < N; ++k) off[k] = sub_off(k, N, a.phase_center);
    for (int yy = wave; yy < TEXT_TILE_H; yy += TEXT_WAVES) {
        const int Y = (int)tl.y0 + yy;
        if (Y >= (int)rn.h) break;
        uint32_t *px = reinterpret_cast<uint32_t *>(a.out) + ((uint64_t)rn.out_y + (uint64_t)Y) * a.out_stride + rn.out_x + (uint32_t)X;
        uint32_t start = rn.clear;                                         // what every sample holds before the first instance
        if constexpr (LOAD) start = X < (int)rn.w ? *px : 0u;             // (X < w, Y < h: the store's guard)
        // channel sums.  RGBA: c0 = R | B << 16, c1 = G | A << 16.  sRGB: linear R, G, B (<= 16 * 65535) and alpha
        uint32_t c0 = 0u, c1 = 0u, c2 = 0u, c3 = 0u;
        bool keep = false;                                                 // (LOAD) every sample untaken: the pixel stays
        if constexpr (BLEND == 0) {
            uint32_t taken = 0u;
            for (uint32_t q = tl.lend; q > tl.lbeg;) {
                const TextInstEx in = a.insts[a.list[--q]];
                if (Y < in.y0 || Y >= in.y1) continue;                   // (wave-uniform)
                const bool inside = X >= in.x0 && X < in.x1;
#include "fr_text_place_mask_kernel.inc"
                if (inside) {
                    const uint32_t k = (uint32_t)__builtin_popcount(m & ~taken);
                    if constexpr (SRGB) {
                        c0 += k * (in.pad[0] & 0xffffu);
                        c1 += k * (in.pad[0] >> 16);
                        c2 += k * in.pad[1];
                        c3 += k * (in.rgba >> 24);
                    } else {
                        c0 += k * (in.rgba & M2);
                        c1 += k * ((in.rgba >> 8) & M2);
                    }
                    taken |= m;
                }
            }
            const uint32_t k = (uint32_t)__builtin_popcount(~taken & FULL);
            if constexpr (SRGB && LOAD) {
                c0 += k * D[start & 0xffu];
                c1 += k * D[(start >> 8) & 0xffu];
                c2 += k * D[(start >> 16) & 0xffu];
                c3 += k * (start >> 24);
            } else if constexpr (SRGB) {
                c0 += k * (rn.pad[0] & 0xffffu);
                c1 += k * (rn.pad[0] >> 16);
                c2 += k * rn.pad[1];
                c3 += k * (start >> 24);
            } else {
                c0 += k * (start & M2);
                c1 += k * ((start >> 8) & M2);
            }
            keep = LOAD && taken == 0u;
        } else {
            uint32_t smp[NN];
#pragma unroll
            for (uint32_t k = 0; k < NN; ++k) smp[k] = start;
            for (uint32_t q = tl.lbeg; q < tl.lend; ++q) {
                const TextInstEx in = a.insts[a.list[q]];
                if (Y < in.y0 || Y >= in.y1) continue;                   // (wave-uniform)
                const bool inside = X >= in.x0 && X < in.x1;
#include "fr_text_place_mask_kernel.inc"
                const uint32_t hit = inside ? m : 0u;
                const uint32_t A = in.rgba >> 24, ia = 255u - A, hiA = in.rgba & 0xff000000u;
                if constexpr (SRGB) {
                    const uint32_t rA = (in.pad[0] & 0xffffu) * A + 127u, gA = (in.pad[0] >> 16) * A + 127u, bA = in.pad[1] * A + 127u;
#pragma unroll
                    for (uint32_t k = 0; k < NN; ++k) {
                        if (hit >> k & 1u) {
                            const uint32_t sm = smp[k];
                            const uint32_t r = place_srgb_encode(K, place_div255_24(rA + (uint32_t)D[sm & 0xffu] * ia));
                            const uint32_t g = place_srgb_encode(K, place_div255_24(gA + (uint32_t)D[(sm >> 8) & 0xffu] * ia));
                            const uint32_t b = place_srgb_encode(K, place_div255_24(bA + (uint32_t)D[(sm >> 16) & 0xffu] * ia));
                            smp[k] = r | g << 8 | b << 16 | hiA;
                        }
                    }
                } else {
                    const uint32_t rbA = (in.rgba & M2) * A + 0x00800080u, gA = ((in.rgba >> 8) & 0xffu) * A + 128u;
#pragma unroll
                    for (uint32_t k = 0; k < NN; ++k) {
                        if (hit >> k & 1u)
                            smp[k] = place_blend2(smp[k] & M2, rbA, ia) | (place_blend2((smp[k] >> 8) & 0xffu, gA, ia) << 8) | hiA;
                    }
                }
            }
#pragma unroll
            for (uint32_t k = 0; k < NN; ++k) {
                if constexpr (SRGB) {
                    c0 += D[smp[k] & 0xffu];
                    c1 += D[(smp[k] >> 8) & 0xffu];
                    c2 += D[(smp[k] >> 16) & 0xffu];
                    c3 += smp[k] >> 24;
                } else {
                    c0 += smp[k] & M2;                                     // at most 16 * 255 per half
                    c1 += (smp[k] >> 8) & M2;
                }
            }
        }
        if (X < (int)rn.w && !keep) {
            uint32_t v;
            if constexpr (SRGB) {
                constexpr uint32_t HALF = NN / 2u;
                v = place_srgb_encode(K, (c0 + HALF) >> LG) | place_srgb_encode(K, (c1 + HALF) >> LG) << 8 |
                    place_srgb_encode(K, (c2 + HALF) >> LG) << 16 | ((c3 + HALF) >> LG) << 24;
            } else {
                constexpr uint32_t HALF = (NN / 2u) * 0x00010001u;
                v = (((c0 + HALF) >> LG) & M2) | ((((c1 + HALF) >> LG) & M2) << 8);
            }
            __builtin_nontemporal_store(v, px);
        }
    }
}

// the sRGB tables into LDS, once per workgroup (as text_srgb_kernel)
#define FR_PLACE_SRGB_TABLES                                                                                            \
    __shared__ uint4 lds_d[sizeof SRGB_D / 16], lds_k[sizeof SRGB_K / 16];                                              \
    for (uint32_t i = threadIdx.x; i < sizeof SRGB_K / 16; i += 64 * TEXT_WAVES)                                        \
        lds_k[i] = reinterpret_cast<const uint4 *>(SRGB_K)[i];                                                          \
    if (threadIdx.x < sizeof SRGB_D / 16) lds_d[threadIdx.x] = reinterpret_cast<const uint4 *>(SRGB_D)[threadIdx.x];    \
    __syncthreads();                                                                                                    \
    const uint16_t *D = reinterpret_cast<const uint16_t *>(lds_d);                                                      \
    const uint16_t *K = reinterpret_cast<const uint16_t *>(lds_k)

template <int N, int FILL, int BLEND>
__global__ __launch_bounds__(64 * TEXT_WAVES) void text_place_rgba_kernel(TextPlaceArgs a)
{
    place_colour_rows<N, FILL, BLEND, false, false>(a, nullptr, nullptr);
}

template <int N, int FILL, int BLEND>
__global__ __launch_bounds__(64 * TEXT_WAVES) void text_place_rgba_load_kernel(TextPlaceArgs a)
{
    place_colour_rows<N, FILL, BLEND, false, true>(a, nullptr, nullptr);
}

template <int N, int FILL, int BLEND>
__global__ __launch_bounds__(64 * TEXT_WAVES) void text_place_srgb_kernel(TextPlaceArgs a)
{
    FR_PLACE_SRGB_TABLES;
    place_colour_rows<N, FILL, BLEND, true, false>(a, D, K);
}

template <int N, int FILL, int BLEND>
__global__ __launch_bounds__(64 * TEXT_WAVES) void text_place_srgb_load_kernel(TextPlaceArgs a)
{
    FR_PLACE_SRGB_TABLES;
    place_colour_rows<N, FILL, BLEND, true, true>(a, D, K);
}

// FAM: 0 coverage, 1 rgba, 2 srgb, 3 rgba load, 4 srgb load (BLEND is 0 for coverage)
template <int N, int FILL, int BLEND, int FAM>
static hipError_t place_launch_n(const TextPlaceArgs &a, uint32_t n_tiles, hipStream_t stream, char *name, size_t name_cap)
{
    static const char *const fam[5] = {"", "rgba_", "srgb_", "rgba_load_", "srgb_load_"};
    if (name) {                                                            // as rocprofv3 names the instance
        if (FAM == 0) snprintf(name, name_cap, "fr::text_place_kernel<%d, %d>", N, FILL);
        else snprintf(name, name_cap, "fr::text_place_%skernel<%d, %d, %d>", fam[FAM], N, FILL, BLEND);
    }
    if (!n_tiles) return hipSuccess;
    const dim3 grid(n_tiles), block(64 * TEXT_WAVES);
    if constexpr (FAM == 0) hipLaunchKernelGGL((text_place_kernel<N, FILL>), grid, block, 0, stream, a);
    else if constexpr (FAM == 1) hipLaunchKernelGGL((text_place_rgba_kernel<N, FILL, BLEND>), grid, block, 0, stream, a);
    else if constexpr (FAM == 2) hipLaunchKernelGGL((text_place_srgb_kernel<N, FILL, BLEND>), grid, block, 0, stream, a);
    else if constexpr (FAM == 3) hipLaunchKernelGGL((text_place_rgba_load_kernel<N, FILL, BLEND>), grid, block, 0, stream, a);
    else hipLaunchKernelGGL((text_place_srgb_load_kernel<N, FILL, BLEND>), grid, block, 0, stream, a);
    return hipGetLastError();
}

template <int FILL, int BLEND, int FAM>
static hipError_t place_launch_fb(const TextPlaceArgs &a, int n, uint32_t n_tiles, hipStream_t stream, char *name, size_t name_cap)
{
    if (n == 4) return place_launch_n<4, FILL, BLEND, FAM>(a, n_tiles, stream, name, name_cap);
    if (n == 2) return place_launch_n<2, FILL, BLEND, FAM>(a, n_tiles, stream, name, name_cap);
    return place_launch_n<1, FILL, BLEND, FAM>(a, n_tiles, stream, name, name_cap);
}

template <int FAM>
static hipError_t place_launch_fam(const TextPlaceArgs &a, int n, int fill, int blend, uint32_t n_tiles, hipStream_t stream,
                                   char *name, size_t name_cap)
{
    if constexpr (FAM == 0) {
        return fill ? place_launch_fb<1, 0, 0>(a, n, n_tiles, stream, name, name_cap)
                    : place_launch_fb<0, 0, 0>(a, n, n_tiles, stream, name, name_cap);
    } else {
        if (fill) return blend ? place_launch_fb<1, 1, FAM>(a, n, n_tiles, stream, name, name_cap)
                               : place_launch_fb<1, 0, FAM>(a, n, n_tiles, stream, name, name_cap);
        return blend ? place_launch_fb<0, 1, FAM>(a, n, n_tiles, stream, name, name_cap)
                     : place_launch_fb<0, 0, FAM>(a, n, n_tiles, stream, name, name_cap);
    }
}

hipError_t launch_text_place(const TextPlaceArgs &a, int n, int fill, int rgba, int blend, int srgb, int load, uint32_t n_tiles,
                             hipStream_t stream, char *name, size_t name_cap)
{
    if (!rgba) return place_launch_fam<0>(a, n, fill, 0, n_tiles, stream, name, name_cap);
    if (load) return srgb ? place_launch_fam<4>(a, n, fill, blend, n_tiles, stream, name, name_cap)
                          : place_launch_fam<3>(a, n, fill, blend, n_tiles, stream, name, name_cap);
    return srgb ? place_launch_fam<2>(a, n, fill, blend, n_tiles, stream, name, name_cap)
                : place_launch_fam<1>(a, n, fill, blend, n_tiles, stream, name, name_cap);
}

}  // namespace fr

// fr_text.hip — text runs (include/fr_raster.h, DESIGN.md sections 4.7 and 5): the union over overlapping glyph
// instances of the non-zero test, per sample, composited into each run's image in one pass.
//
// One workgroup of four waves takes one TILE of a run: 64 image columns x 16 image rows; a wave takes every fourth row
// of it, one pixel per lane.  The plan lists, once on the host, the instances whose (clipped) cells meet each tile.  For
// one row and one instance every ray height cy is the same in all lanes, so the root of each record — the reference's
// own arithmetic (rec_cross, fr_device.hpp) — is wave-uniform and only the crossing test !(xx < cx) is per lane: n^2
// winding counters per lane, reduced to an n^2-bit mask (winding != 0) that is ORed over the instances whose cell
// contains the pixel.  The records are the stand-alone ones of prepare_kernel (fr_prepare.hip), rebuilt from the glyph
// points into plan-owned memory before every render, so a glyph of any size takes this path.  Every pixel of the run is
// written (0 where no instance reaches), a wave's row as 64 consecutive bytes, stored non-temporally.
//
// text_rgba_kernel is the same work layout for RGBA text plans: the same per-instance mask (fr_text_mask_kernel.inc), but
// each lane applies the instances' colours to its n^2 samples in placement order and writes one RGBA dword per pixel, a
// wave's row as 256 consecutive bytes.  text_srgb_kernel is text_rgba_kernel for FR_TEXT_SRGB plans: it blends and
// resolves in 16-bit linear light through the tables of fr_srgb.hpp, copied into LDS once per workgroup.
// text_rgba_load_kernel and text_srgb_load_kernel are those two for FR_TEXT_LOAD plans: the samples start at the pixel
// already in the output, and only the tiles under some instance are launched.
#include "fr_text.hpp"
#include "fr_srgb.hpp"

#include <cstdio>

namespace fr {

template <int N, int FILL>
__global__ __launch_bounds__(64 * TEXT_WAVES) void text_kernel(TextArgs a)
{
    const TextTile tl = a.tiles[blockIdx.x];
    const TextRun rn = a.runs[tl.run];
    const int lane = (int)(threadIdx.x & 63u);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int X = (int)tl.x0 + lane;
    const float scale = rn.scale;
    float off[N];
#pragma unroll
    for (int k = 0; k < N; ++k) off[k] = sub_off(k, N, a.phase_center);
    for (int yy = wave; yy < TEXT_TILE_H; yy += TEXT_WAVES) {
        const int Y = (int)tl.y0 + yy;
        if (Y >= (int)rn.h) break;
        uint32_t mask = 0u;
        for (uint32_t q = tl.lbeg; q < tl.lend; ++q) {
            const TextInst in = a.insts[a.list[q]];
            if (Y < in.y0 || Y >= in.y1) continue;                       // (wave-uniform)
            const bool inside = X >= in.x0 && X < in.x1;
#include "fr_text_mask_kernel.inc"
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

template <int N, int FILL>
static hipError_t text_launch_n(const TextArgs &a, uint32_t n_tiles, hipStream_t stream, char *name, size_t name_cap)
{
    if (name) snprintf(name, name_cap, "fr::text_kernel<%d, %d>", N, FILL);      // as rocprofv3 names the instance
    if (!n_tiles) return hipSuccess;
    hipLaunchKernelGGL((text_kernel<N, FILL>), dim3(n_tiles), dim3(64 * TEXT_WAVES), 0, stream, a);
    return hipGetLastError();
}

template <int FILL>
static hipError_t text_launch_fill(const TextArgs &a, int n, uint32_t n_tiles, hipStream_t stream, char *name, size_t name_cap)
{
    if (n == 4) return text_launch_n<4, FILL>(a, n_tiles, stream, name, name_cap);
    if (n == 2) return text_launch_n<2, FILL>(a, n_tiles, stream, name, name_cap);
    return text_launch_n<1, FILL>(a, n_tiles, stream, name, name_cap);
}

hipError_t launch_text(const TextArgs &a, int n, int fill, uint32_t n_tiles, hipStream_t stream, char *name, size_t name_cap)
{
    if (fill) return text_launch_fill<1>(a, n, n_tiles, stream, name, name_cap);
    return text_launch_fill<0>(a, n, n_tiles, stream, name, name_cap);
}

// ---- RGBA text plans (fr_text_plan_create_rgba) ---------------------------------------------------------------------
// Two 8-bit channels at once, in bits 0-7 and 16-23 of a word: (x + 127) div 255 with x = C*A + c*(255 - A) in [0, 65025]
// as (t + (t >> 8)) >> 8, t = x + 128 (exact over that whole domain: tests/test_text_rgba_ref.py checks every x).
// t + (t >> 8) < 2^16, so the halves never carry into each other.  c2: the sample's two channels; cA2 = C2 * A + 128 each.
__device__ __forceinline__ uint32_t blend2(uint32_t c2, uint32_t cA2, uint32_t ia)
{
    const uint32_t t = c2 * ia + cA2;
    return ((t + ((t >> 8) & 0x00ff00ffu)) >> 8) & 0x00ff00ffu;
}

// BLEND = 0: every placement colour is opaque, so a sample takes the colour of the last instance that covers it (or the
// clear colour): the instances are walked backwards and each adds the samples it takes first.  BLEND = 1: n^2 RGBA8
// sample states per lane, blended forwards in placement order (src*A + dst*(255 - A) for R G B, alpha replaced by A).
// Either way the pixel is (sum over the samples + n^2/2) div n^2 per channel.  (text_rgba_load_kernel, below, is this
// kernel for FR_TEXT_LOAD plans: keep the two in step.)
template <int N, int FILL, int BLEND>
__global__ __launch_bounds__(64 * TEXT_WAVES) void text_rgba_kernel(TextArgs a)
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
    const float scale = rn.scale;
    float off[N];
#pragma unroll
    for (int k = 0; k < N; ++k) off[k] = sub_off(k, N, a.phase_center);
    for (int yy = wave; yy < TEXT_TILE_H; yy += TEXT_WAVES) {
        const int Y = (int)tl.y0 + yy;
        if (Y >= (int)rn.h) break;
        uint32_t rb, ga;                                                   // channel sums: R | B << 16, G | A << 16
        if constexpr (BLEND == 0) {
            uint32_t taken = 0u;
            rb = 0u;
            ga = 0u;
            for (uint32_t q = tl.lend; q > tl.lbeg;) {
                const TextInst in = a.insts[a.list[--q]];
                if (Y < in.y0 || Y >= in.y1) continue;                   // (wave-uniform)
                const bool inside = X >= in.x0 && X < in.x1;
#include "fr_text_mask_kernel.inc"
                if (inside) {
                    const uint32_t k = (uint32_t)__builtin_popcount(m & ~taken);
                    rb += k * (in.rgba & M2);
                    ga += k * ((in.rgba >> 8) & M2);
                    taken |= m;
                }
            }
            const uint32_t k = (uint32_t)__builtin_popcount(~taken & FULL);
            rb += k * (rn.clear & M2);
            ga += k * ((rn.clear >> 8) & M2);
        } else {
            uint32_t smp[NN];
#pragma unroll
            for (uint32_t k = 0; k < NN; ++k) smp[k] = rn.clear;
            for (uint32_t q = tl.lbeg; q < tl.lend; ++q) {
                const TextInst in = a.insts[a.list[q]];
                if (Y < in.y0 || Y >= in.y1) continue;                   // (wave-uniform)
                const bool inside = X >= in.x0 && X < in.x1;
#include "fr_text_mask_kernel.inc"
                const uint32_t hit = inside ? m : 0u;
                const uint32_t A = in.rgba >> 24, ia = 255u - A, hiA = in.rgba & 0xff000000u;
                const uint32_t rbA = (in.rgba & M2) * A + 0x00800080u, gA = ((in.rgba >> 8) & 0xffu) * A + 128u;
#pragma unroll
                for (uint32_t k = 0; k < NN; ++k) {
                    if (hit >> k & 1u)
                        smp[k] = blend2(smp[k] & M2, rbA, ia) | (blend2((smp[k] >> 8) & 0xffu, gA, ia) << 8) | hiA;
                }
            }
            rb = 0u;
            ga = 0u;
#pragma unroll
            for (uint32_t k = 0; k < NN; ++k) {
                rb += smp[k] & M2;                                         // at most 16 * 255 per half
                ga += (smp[k] >> 8) & M2;
            }
        }
        if (X < (int)rn.w) {
            constexpr uint32_t HALF = (NN / 2u) * 0x00010001u;
            const uint32_t v = (((rb + HALF) >> LG) & M2) | ((((ga + HALF) >> LG) & M2) << 8);
            uint32_t *dst = reinterpret_cast<uint32_t *>(a.out) + ((uint64_t)rn.out_y + (uint64_t)Y) * a.out_stride + rn.out_x + (uint32_t)X;
            __builtin_nontemporal_store(v, dst);
        }
    }
}

template <int N, int FILL, int BLEND>
static hipError_t text_rgba_launch_n(const TextArgs &a, uint32_t n_tiles, hipStream_t stream, char *name, size_t name_cap)
{
    if (name) snprintf(name, name_cap, "fr::text_rgba_kernel<%d, %d, %d>", N, FILL, BLEND);      // as rocprofv3 names it
    if (!n_tiles) return hipSuccess;
    hipLaunchKernelGGL((text_rgba_kernel<N, FILL, BLEND>), dim3(n_tiles), dim3(64 * TEXT_WAVES), 0, stream, a);
    return hipGetLastError();
}

template <int FILL, int BLEND>
static hipError_t text_rgba_launch_fb(const TextArgs &a, int n, uint32_t n_tiles, hipStream_t stream, char *name, size_t name_cap)
{
    if (n == 4) return text_rgba_launch_n<4, FILL, BLEND>(a, n_tiles, stream, name, name_cap);
    if (n == 2) return text_rgba_launch_n<2, FILL, BLEND>(a, n_tiles, stream, name, name_cap);
    return text_rgba_launch_n<1, FILL, BLEND>(a, n_tiles, stream, name, name_cap);
}

hipError_t launch_text_rgba(const TextArgs &a, int n, int fill, int blend, uint32_t n_tiles, hipStream_t stream, char *name,
                            size_t name_cap)
{
    if (fill) return blend ? text_rgba_launch_fb<1, 1>(a, n, n_tiles, stream, name, name_cap)
                           : text_rgba_launch_fb<1, 0>(a, n, n_tiles, stream, name, name_cap);
    return blend ? text_rgba_launch_fb<0, 1>(a, n, n_tiles, stream, name, name_cap)
                 : text_rgba_launch_fb<0, 0>(a, n, n_tiles, stream, name, name_cap);
}

// ---- sRGB text plans (fr_text_plan_create_rgba with FR_TEXT_SRGB) --------------------------------------------------
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

// BLEND = 0: every placement colour is opaque, so a sample holds the colour of the last instance that covers it (or the
// clear colour), whose linear value the host put in TextInst::pad / TextRun::pad: the instances are walked backwards
// and each adds k * D[C] per channel for the k samples it takes first.  BLEND = 1: n^2 sRGB RGBA8 sample states per
// lane, blended forwards in placement order, c' = E((D[C] * A + D[c] * (255 - A) + 127) div 255) for R G B, alpha
// replaced by A.  Either way the pixel is E((sum over the samples of D[c] + n^2/2) div n^2) per colour channel and
// (sum of a + n^2/2) div n^2 for alpha.  (text_srgb_load_kernel, below, is this kernel for FR_TEXT_LOAD plans: keep the
// two in step.)
template <int N, int FILL, int BLEND>
__global__ __launch_bounds__(64 * TEXT_WAVES) void text_srgb_kernel(TextArgs a)
{
    constexpr uint32_t NN = (uint32_t)(N * N);
    constexpr uint32_t FULL = NN == 32u ? ~0u : (1u << NN) - 1u;
    constexpr uint32_t LG = N == 4 ? 4u : N == 2 ? 2u : 0u;              // log2(n^2)
    constexpr uint32_t HALF = NN / 2u;
    __shared__ uint4 lds_d[sizeof SRGB_D / 16], lds_k[sizeof SRGB_K / 16];
    for (uint32_t i = threadIdx.x; i < sizeof SRGB_K / 16; i += 64 * TEXT_WAVES)
        lds_k[i] = reinterpret_cast<const uint4 *>(SRGB_K)[i];
    if (threadIdx.x < sizeof SRGB_D / 16) lds_d[threadIdx.x] = reinterpret_cast<const uint4 *>(SRGB_D)[threadIdx.x];
    __syncthreads();
    const uint16_t *D = reinterpret_cast<const uint16_t *>(lds_d);
    const uint16_t *K = reinterpret_cast<const uint16_t *>(lds_k);
    const TextTile tl = a.tiles[blockIdx.x];
    const TextRun rn = a.runs[tl.run];
    const int lane = (int)(threadIdx.x & 63u);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int X = (int)tl.x0 + lane;
    const float scale = rn.scale;
    float off[N];
#pragma unroll
    for (int k = 0; k < N; ++k) off[k] = sub_off(k, N, a.phase_center);
    for (int yy = wave; yy < TEXT_TILE_H; yy += TEXT_WAVES) {
        const int Y = (int)tl.y0 + yy;
        if (Y >= (int)rn.h) break;
        uint32_t sr = 0u, sg = 0u, sb = 0u, sa = 0u;                     // linear R G B sums (<= 16 * 65535), alpha sum
        if constexpr (BLEND == 0) {
            uint32_t taken = 0u;
            for (uint32_t q = tl.lend; q > tl.lbeg;) {
                const TextInst in = a.insts[a.list[--q]];
                if (Y < in.y0 || Y >= in.y1) continue;                   // (wave-uniform)
                const bool inside = X >= in.x0 && X < in.x1;
#include "fr_text_mask_kernel.inc"
                if (inside) {
                    const uint32_t k = (uint32_t)__builtin_popcount(m & ~taken);
                    sr += k * (in.pad[0] & 0xffffu);
                    sg += k * (in.pad[0] >> 16);
                    sb += k * in.pad[1];
                    sa += k * (in.rgba >> 24);
                    taken |= m;
                }
            }
            const uint32_t k = (uint32_t)__builtin_popcount(~taken & FULL);
            sr += k * (rn.pad[0] & 0xffffu);
            sg += k * (rn.pad[0] >> 16);
            sb += k * rn.pad[1];
            sa += k * (rn.clear >> 24);
        } else {
            uint32_t smp[NN];
#pragma unroll
            for (uint32_t k = 0; k < NN; ++k) smp[k] = rn.clear;
            for (uint32_t q = tl.lbeg; q < tl.lend; ++q) {
                const TextInst in = a.insts[a.list[q]];
                if (Y < in.y0 || Y >= in.y1) continue;                   // (wave-uniform)
                const bool inside = X >= in.x0 && X < in.x1;
#include "fr_text_mask_kernel.inc"
                const uint32_t hit = inside ? m : 0u;
                const uint32_t A = in.rgba >> 24, ia = 255u - A, hiA = in.rgba & 0xff000000u;
                const uint32_t rA = (in.pad[0] & 0xffffu) * A + 127u, gA = (in.pad[0] >> 16) * A + 127u, bA = in.pad[1] * A + 127u;
#pragma unroll
                for (uint32_t k = 0; k < NN; ++k) {
                    if (hit >> k & 1u) {
                        const uint32_t s = smp[k];
                        const uint32_t r = srgb_encode(K, div255_24(rA + (uint32_t)D[s & 0xffu] * ia));
                        const uint32_t g = srgb_encode(K, div255_24(gA + (uint32_t)D[(s >> 8) & 0xffu] * ia));
                        const uint32_t b = srgb_encode(K, div255_24(bA + (uint32_t)D[(s >> 16) & 0xffu] * ia));
                        smp[k] = r | g << 8 | b << 16 | hiA;
                    }
                }
            }
#pragma unroll
            for (uint32_t k = 0; k < NN; ++k) {
                sr += D[smp[k] & 0xffu];
                sg += D[(smp[k] >> 8) & 0xffu];
                sb += D[(smp[k] >> 16) & 0xffu];
                sa += smp[k] >> 24;
            }
        }
        if (X < (int)rn.w) {
            const uint32_t v = srgb_encode(K, (sr + HALF) >> LG) | srgb_encode(K, (sg + HALF) >> LG) << 8 |
                               srgb_encode(K, (sb + HALF) >> LG) << 16 | ((sa + HALF) >> LG) << 24;
            uint32_t *dst = reinterpret_cast<uint32_t *>(a.out) + ((uint64_t)rn.out_y + (uint64_t)Y) * a.out_stride + rn.out_x + (uint32_t)X;
            __builtin_nontemporal_store(v, dst);
        }
    }
}

template <int N, int FILL, int BLEND>
static hipError_t text_srgb_launch_n(const TextArgs &a, uint32_t n_tiles, hipStream_t stream, char *name, size_t name_cap)
{
    if (name) snprintf(name, name_cap, "fr::text_srgb_kernel<%d, %d, %d>", N, FILL, BLEND);      // as rocprofv3 names it
    if (!n_tiles) return hipSuccess;
    hipLaunchKernelGGL((text_srgb_kernel<N, FILL, BLEND>), dim3(n_tiles), dim3(64 * TEXT_WAVES), 0, stream, a);
    return hipGetLastError();
}

template <int FILL, int BLEND>
static hipError_t text_srgb_launch_fb(const TextArgs &a, int n, uint32_t n_tiles, hipStream_t stream, char *name, size_t name_cap)
{
    if (n == 4) return text_srgb_launch_n<4, FILL, BLEND>(a, n_tiles, stream, name, name_cap);
    if (n == 2) return text_srgb_launch_n<2, FILL, BLEND>(a, n_tiles, stream, name, name_cap);
    return text_srgb_launch_n<1, FILL, BLEND>(a, n_tiles, stream, name, name_cap);
}

hipError_t launch_text_srgb(const TextArgs &a, int n, int fill, int blend, uint32_t n_tiles, hipStream_t stream, char *name,
                            size_t name_cap)
{
    if (fill) return blend ? text_srgb_launch_fb<1, 1>(a, n, n_tiles, stream, name, name_cap)
                           : text_srgb_launch_fb<1, 0>(a, n, n_tiles, stream, name, name_cap);
    return blend ? text_srgb_launch_fb<0, 1>(a, n, n_tiles, stream, name, name_cap)
                 : text_srgb_launch_fb<0, 0>(a, n, n_tiles, stream, name, name_cap);
}

// ---- FR_TEXT_LOAD: RGBA and sRGB text plans drawn over the pixels already in the output ------------------------------
// text_rgba_load_kernel / text_srgb_load_kernel are text_rgba_kernel / text_srgb_kernel with one change: every sample of
// a pixel starts at the pixel's value in the output instead of the run's clear colour.  Each lane loads its pixel (one
// dword, guarded as the store is) before the instance walk, so the load's latency hides under the wave-uniform root
// evaluations.  BLEND = 0: the samples no instance takes add k * dst per channel; a lane whose samples are all untaken
// holds dst exactly (the resolve of n^2 equal values; for sRGB E(D[v]) = v), so it skips its store and the row costs
// only the reads where no glyph reaches.  BLEND = 1: smp[k] = dst, and every pixel of the tile is stored.  The plan
// launches only the tiles whose instance list is non-empty (fr_api.hip): every pixel of the run in a launched tile is
// read, and a pixel of any other tile is neither read nor written.
// KEEP IN STEP: apart from the start value (dst for rn.clear / rn.pad, with its load) and the store skip, these two are
// line for line text_rgba_kernel and text_srgb_kernel; a change to one pair's walk, blend or resolve belongs in the other.
// (They are copies rather than one body with a LOAD parameter because such a shared inline body changes the scheduled
// assembly of the existing kernels, whose code this flag must leave as it is.)
// FR_TEXT_LOAD_SKIP=0 (an experiment build only: make variant) stores every pixel, to price the skip.
#ifndef FR_TEXT_LOAD_SKIP
#define FR_TEXT_LOAD_SKIP 1
#endif
template <int N, int FILL, int BLEND>
__global__ __launch_bounds__(64 * TEXT_WAVES) void text_rgba_load_kernel(TextArgs a)
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
    const float scale = rn.scale;
    float off[N];
#pragma unroll
    for (int k = 0; k < N; ++k) off[k] = sub_off(k, N, a.phase_center);
    for (int yy = wave; yy < TEXT_TILE_H; yy += TEXT_WAVES) {
        const int Y = (int)tl.y0 + yy;
        if (Y >= (int)rn.h) break;
        uint32_t *px = reinterpret_cast<uint32_t *>(a.out) + ((uint64_t)rn.out_y + (uint64_t)Y) * a.out_stride + rn.out_x + (uint32_t)X;
        const uint32_t dst = X < (int)rn.w ? *px : 0u;                   // (X < w, Y < h: the store's guard)
        uint32_t rb, ga;                                                   // channel sums: R | B << 16, G | A << 16
        bool keep = false;                                                 // every sample untaken: the pixel stays dst
        if constexpr (BLEND == 0) {
            uint32_t taken = 0u;
            rb = 0u;
            ga = 0u;
            for (uint32_t q = tl.lend; q > tl.lbeg;) {
                const TextInst in = a.insts[a.list[--q]];
                if (Y < in.y0 || Y >= in.y1) continue;                   // (wave-uniform)
                const bool inside = X >= in.x0 && X < in.x1;
#include "fr_text_mask_kernel.inc"
                if (inside) {
                    const uint32_t k = (uint32_t)__builtin_popcount(m & ~taken);
                    rb += k * (in.rgba & M2);
                    ga += k * ((in.rgba >> 8) & M2);
                    taken |= m;
                }
            }
            const uint32_t k = (uint32_t)__builtin_popcount(~taken & FULL);
            rb += k * (dst & M2);
            ga += k * ((dst >> 8) & M2);
            keep = FR_TEXT_LOAD_SKIP && taken == 0u;
        } else {
            uint32_t smp[NN];
#pragma unroll
            for (uint32_t k = 0; k < NN; ++k) smp[k] = dst;
            for (uint32_t q = tl.lbeg; q < tl.lend; ++q) {
                const TextInst in = a.insts[a.list[q]];
                if (Y < in.y0 || Y >= in.y1) continue;                   // (wave-uniform)
                const bool inside = X >= in.x0 && X < in.x1;
#include "fr_text_mask_kernel.inc"
                const uint32_t hit = inside ? m : 0u;
                const uint32_t A = in.rgba >> 24, ia = 255u - A, hiA = in.rgba & 0xff000000u;
                const uint32_t rbA = (in.rgba & M2) * A + 0x00800080u, gA = ((in.rgba >> 8) & 0xffu) * A + 128u;
#pragma unroll
                for (uint32_t k = 0; k < NN; ++k) {
                    if (hit >> k & 1u)
                        smp[k] = blend2(smp[k] & M2, rbA, ia) | (blend2((smp[k] >> 8) & 0xffu, gA, ia) << 8) | hiA;
                }
            }
            rb = 0u;
            ga = 0u;
#pragma unroll
            for (uint32_t k = 0; k < NN; ++k) {
                rb += smp[k] & M2;                                         // at most 16 * 255 per half
                ga += (smp[k] >> 8) & M2;
            }
        }
        if (X < (int)rn.w && !keep) {
            constexpr uint32_t HALF = (NN / 2u) * 0x00010001u;
            const uint32_t v = (((rb + HALF) >> LG) & M2) | ((((ga + HALF) >> LG) & M2) << 8);
            __builtin_nontemporal_store(v, px);
        }
    }
}

// text_srgb_kernel over the output's pixels: the untaken samples add k * D[dst.c] (BLEND = 0), or start at dst (BLEND = 1)
template <int N, int FILL, int BLEND>
__global__ __launch_bounds__(64 * TEXT_WAVES) void text_srgb_load_kernel(TextArgs a)
{
    constexpr uint32_t NN = (uint32_t)(N * N);
    constexpr uint32_t FULL = NN == 32u ? ~0u : (1u << NN) - 1u;
    constexpr uint32_t LG = N == 4 ? 4u : N == 2 ? 2u : 0u;              // log2(n^2)
    constexpr uint32_t HALF = NN / 2u;
    __shared__ uint4 lds_d[sizeof SRGB_D / 16], lds_k[sizeof SRGB_K / 16];
    for (uint32_t i = threadIdx.x; i < sizeof SRGB_K / 16; i += 64 * TEXT_WAVES)
        lds_k[i] = reinterpret_cast<const uint4 *>(SRGB_K)[i];
    if (threadIdx.x < sizeof SRGB_D / 16) lds_d[threadIdx.x] = reinterpret_cast<const uint4 *>(SRGB_D)[threadIdx.x];
    __syncthreads();
    const uint16_t *D = reinterpret_cast<const uint16_t *>(lds_d);
    const uint16_t *K = reinterpret_cast<const uint16_t *>(lds_k);
    const TextTile tl = a.tiles[blockIdx.x];
    const TextRun rn = a.runs[tl.run];
    const int lane = (int)(threadIdx.x & 63u);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int X = (int)tl.x0 + lane;
    const float scale = rn.scale;
    float off[N];
#pragma unroll
    for (int k = 0; k < N; ++k) off[k] = sub_off(k, N, a.phase_center);
    for (int yy = wave; yy < TEXT_TILE_H; yy += TEXT_WAVES) {
        const int Y = (int)tl.y0 + yy;
        if (Y >= (int)rn.h) break;
        uint32_t *px = reinterpret_cast<uint32_t *>(a.out) + ((uint64_t)rn.out_y + (uint64_t)Y) * a.out_stride + rn.out_x + (uint32_t)X;
        const uint32_t dst = X < (int)rn.w ? *px : 0u;                   // (X < w, Y < h: the store's guard)
        uint32_t sr = 0u, sg = 0u, sb = 0u, sa = 0u;                     // linear R G B sums (<= 16 * 65535), alpha sum
        bool keep = false;                                                 // every sample untaken: the pixel stays dst
        if constexpr (BLEND == 0) {
            uint32_t taken = 0u;
            for (uint32_t q = tl.lend; q > tl.lbeg;) {
                const TextInst in = a.insts[a.list[--q]];
                if (Y < in.y0 || Y >= in.y1) continue;                   // (wave-uniform)
                const bool inside = X >= in.x0 && X < in.x1;
#include "fr_text_mask_kernel.inc"
                if (inside) {
                    const uint32_t k = (uint32_t)__builtin_popcount(m & ~taken);
                    sr += k * (in.pad[0] & 0xffffu);
                    sg += k * (in.pad[0] >> 16);
                    sb += k * in.pad[1];
                    sa += k * (in.rgba >> 24);
                    taken |= m;
                }
            }
            const uint32_t k = (uint32_t)__builtin_popcount(~taken & FULL);
            sr += k * D[dst & 0xffu];
            sg += k * D[(dst >> 8) & 0xffu];
            sb += k * D[(dst >> 16) & 0xffu];
            sa += k * (dst >> 24);
            keep = FR_TEXT_LOAD_SKIP && taken == 0u;
        } else {
            uint32_t smp[NN];
#pragma unroll
            for (uint32_t k = 0; k < NN; ++k) smp[k] = dst;
            for (uint32_t q = tl.lbeg; q < tl.lend; ++q) {
                const TextInst in = a.insts[a.list[q]];
                if (Y < in.y0 || Y >= in.y1) continue;                   // (wave-uniform)
                const bool inside = X >= in.x0 && X < in.x1;
#include "fr_text_mask_kernel.inc"
                const uint32_t hit = inside ? m : 0u;
                const uint32_t A = in.rgba >> 24, ia = 255u - A, hiA = in.rgba & 0xff000000u;
                const uint32_t rA = (in.pad[0] & 0xffffu) * A + 127u, gA = (in.pad[0] >> 16) * A + 127u, bA = in.pad[1] * A + 127u;
#pragma unroll
                for (uint32_t k = 0; k < NN; ++k) {
                    if (hit >> k & 1u) {
                        const uint32_t s = smp[k];
                        const uint32_t r = srgb_encode(K, div255_24(rA + (uint32_t)D[s & 0xffu] * ia));
                        const uint32_t g = srgb_encode(K, div255_24(gA + (uint32_t)D[(s >> 8) & 0xffu] * ia));
                        const uint32_t b = srgb_encode(K, div255_24(bA + (uint32_t)D[(s >> 16) & 0xffu] * ia));
                        smp[k] = r | g << 8 | b << 16 | hiA;
                    }
                }
            }
#pragma unroll
            for (uint32_t k = 0; k < NN; ++k) {
                sr += D[smp[k] & 0xffu];
                sg += D[(smp[k] >> 8) & 0xffu];
                sb += D[(smp[k] >> 16) & 0xffu];
                sa += smp[k] >> 24;
            }
        }
        if (X < (int)rn.w && !keep) {
            const uint32_t v = srgb_encode(K, (sr + HALF) >> LG) | srgb_encode(K, (sg + HALF) >> LG) << 8 |
                               srgb_encode(K, (sb + HALF) >> LG) << 16 | ((sa + HALF) >> LG) << 24;
            __builtin_nontemporal_store(v, px);
        }
    }
}

template <int N, int FILL, int BLEND, bool SRGB>
static hipError_t text_load_launch_n(const TextArgs &a, uint32_t n_tiles, hipStream_t stream, char *name, size_t name_cap)
{
    if (name) snprintf(name, name_cap, "fr::text_%s_load_kernel<%d, %d, %d>", SRGB ? "srgb" : "rgba", N, FILL, BLEND);
    if (!n_tiles) return hipSuccess;
    if constexpr (SRGB) hipLaunchKernelGGL((text_srgb_load_kernel<N, FILL, BLEND>), dim3(n_tiles), dim3(64 * TEXT_WAVES), 0, stream, a);
    else hipLaunchKernelGGL((text_rgba_load_kernel<N, FILL, BLEND>), dim3(n_tiles), dim3(64 * TEXT_WAVES), 0, stream, a);
    return hipGetLastError();
}

template <int FILL, int BLEND, bool SRGB>
static hipError_t text_load_launch_fb(const TextArgs &a, int n, uint32_t n_tiles, hipStream_t stream, char *name, size_t name_cap)
{
    if (n == 4) return text_load_launch_n<4, FILL, BLEND, SRGB>(a, n_tiles, stream, name, name_cap);
    if (n == 2) return text_load_launch_n<2, FILL, BLEND, SRGB>(a, n_tiles, stream, name, name_cap);
    return text_load_launch_n<1, FILL, BLEND, SRGB>(a, n_tiles, stream, name, name_cap);
}

template <bool SRGB>
static hipError_t text_load_launch(const TextArgs &a, int n, int fill, int blend, uint32_t n_tiles, hipStream_t stream, char *name,
                                   size_t name_cap)
{
    if (fill) return blend ? text_load_launch_fb<1, 1, SRGB>(a, n, n_tiles, stream, name, name_cap)
                           : text_load_launch_fb<1, 0, SRGB>(a, n, n_tiles, stream, name, name_cap);
    return blend ? text_load_launch_fb<0, 1, SRGB>(a, n, n_tiles, stream, name, name_cap)
                 : text_load_launch_fb<0, 0, SRGB>(a, n, n_tiles, stream, name, name_cap);
}

hipError_t launch_text_load(const TextArgs &a, int n, int fill, int blend, int srgb, uint32_t n_tiles, hipStream_t stream,
                            char *name, size_t name_cap)
{
    return srgb ? text_load_launch<true>(a, n, fill, blend, n_tiles, stream, name, name_cap)
                : text_load_launch<false>(a, n, fill, blend, n_tiles, stream, name, name_cap);
}

}  // namespace fr

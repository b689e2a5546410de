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
// wave's row as 256 consecutive bytes.
#include "fr_text.hpp"

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
// Either way the pixel is (sum over the samples + n^2/2) div n^2 per channel.
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

}  // namespace fr

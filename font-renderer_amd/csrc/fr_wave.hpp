// fr_wave.hpp — wave64 building blocks shared by the three coverage / winding kernels (render_kernel, cov4_kernel,
// win1_kernel): DPP scans, the in-wave LDS hand-off, the packed sorting network and the gray map.
#pragma once
#include "fr_device.hpp"

namespace fr {

// one DPP move with `old` = 0 (lanes whose source is outside the row, or whose row is masked off, read 0)
template <int CTRL, int ROW_MASK = 0xf>
__device__ __forceinline__ uint32_t dpp(uint32_t x)
{
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, CTRL, ROW_MASK, 0xf, false);
}
// wave64 inclusive scans on DPP (row_shr within the 16-lane rows, then row_bcast:15 / :31 carry
// the row totals across rows): 6 VALU operations, no LDS.  `old` = 0 is the identity of both.
__device__ __forceinline__ uint32_t wave_incl_add(uint32_t x)
{
    x += dpp<0x111>(x);                         // row_shr:1
    x += dpp<0x112>(x);                         // row_shr:2
    x += dpp<0x114>(x);                         // row_shr:4
    x += dpp<0x118>(x);                         // row_shr:8
    x += dpp<0x142, 0xa>(x);                    // row_bcast:15 -> rows 1, 3
    x += dpp<0x143, 0xc>(x);                    // row_bcast:31 -> rows 2, 3
    return x;
}
__device__ __forceinline__ uint32_t wave_incl_max(uint32_t x)
{
    x = max(x, dpp<0x111>(x));
    x = max(x, dpp<0x112>(x));
    x = max(x, dpp<0x114>(x));
    x = max(x, dpp<0x118>(x));
    x = max(x, dpp<0x142, 0xa>(x));
    x = max(x, dpp<0x143, 0xc>(x));
    return x;
}

// LDS hand-off inside ONE wave (writer lanes -> reader lanes of the same wave): LDS operations
// of a wave complete in order, so a drained lgkmcnt plus a compiler barrier is enough — no
// s_barrier, the other waves of the workgroup are never waited for.
__device__ __forceinline__ void wave_lds_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// Sorting 2H crossings that sit PACKED two per register (d[j] = slot 2j | slot 2j+1 << 16), ascending:
//   1. Batcher's odd-even merge network over the H registers with v_pk_min_u16 / v_pk_max_u16 — the low
//      halves and the high halves are sorted as two independent sequences by the same instructions;
//   2. one "flip" step merges them (low[j] against high[H-1-j]; a half swap, a packed min/max and two
//      byte permutes per register pair): afterwards every low half <= every high half and both are bitonic;
//   3. log2(H) half-cleaner stages, again packed.
// Result: low halves = s[0..H), high halves = s[H..2H).  About half the instructions of the unpacked
// network, no unpacking, half the registers.
typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void pce(uint32_t &a, uint32_t &b)
{
    const u16x2 x = __builtin_bit_cast(u16x2, a), y = __builtin_bit_cast(u16x2, b);
    a = __builtin_bit_cast(uint32_t, __builtin_elementwise_min(x, y));
    b = __builtin_bit_cast(uint32_t, __builtin_elementwise_max(x, y));
}
template <int H>
__device__ __forceinline__ void packed_sort(uint32_t (&d)[16])
{
#pragma unroll
    for (int p = 1; p < H; p *= 2)
#pragma unroll
        for (int k = p; k >= 1; k /= 2)
#pragma unroll
            for (int j = k % p; j + k < H; j += 2 * k)
#pragma unroll
                for (int i = 0; i < k; ++i)
                    if (i + j + k < H && (i + j) / (2 * p) == (i + j + k) / (2 * p)) pce(d[i + j], d[i + j + k]);
#pragma unroll
    for (int j = 0; j < H / 2; ++j) {
        const uint32_t x = d[j], y = d[H - 1 - j];
        const uint32_t ys = __builtin_amdgcn_alignbit(y, y, 16);                    // halves swapped
        const u16x2 xv = __builtin_bit_cast(u16x2, x), yv = __builtin_bit_cast(u16x2, ys);
        const uint32_t mn = __builtin_bit_cast(uint32_t, __builtin_elementwise_min(xv, yv));
        const uint32_t mx = __builtin_bit_cast(uint32_t, __builtin_elementwise_max(xv, yv));
        d[j] = __builtin_amdgcn_perm(mx, mn, 0x05040100u);                          // min of pair j | max of pair j
        d[H - 1 - j] = __builtin_amdgcn_perm(mx, mn, 0x07060302u);                  // the same of pair H-1-j
    }
#pragma unroll
    for (int k = H / 2; k >= 1; k /= 2)
#pragma unroll
        for (int j = 0; j < H; ++j)
            if (!(j & k)) pce(d[j], d[j + k]);
}

// renderGlyph's gray map of a winding number
__device__ __forceinline__ uint32_t gray_debug(int w)
{
    const int v = w * 20 + 100;                 // render_glyph.zig:28
    return (uint32_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

}  // namespace fr

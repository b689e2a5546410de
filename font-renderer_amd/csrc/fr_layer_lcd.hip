// fr_layer_lcd.hip — sub-pixel (LCD) text: a 3x-wide coverage plane filtered across sub-pixels and composited with one alpha
// per colour byte (fr_layer_lcd; include/fr_raster.h; DESIGN.md sections 4.12 and 5).  Bandwidth-bound like fr_layer.hip
// and fr_layer_paint.hip, whose tile ownership it shares; the pixel arithmetic is over_px_ca of fr_layer_px.hpp.
#include "fr_layer_lcd.hpp"
#include "fr_layer_px.hpp"
#include "fr_srgb.hpp"

namespace fr {

// One workgroup per tile of the table (fr_layer_lcd_plan.hpp), with layer_over_kernel's ownership: lane l of every wave
// owns the four pixels at columns t.x + 4 l .. + 3 of the rows t.y + 4 w .. + 3 of its wave w, and with them the twelve
// plane elements e0 .. e0 + 11, e0 = t.sq + 12 l.  A lane loads those of its elements that lie in the window [t.q0, t.q1),
// whether its pixels belong to the clipped rectangle or not (a clipped-away pixel's sub-pixels are its neighbour's taps):
// as three dwords where the tile's flag says they are aligned and they stay inside the row, masked to the window; byte by
// byte otherwise.  The two taps on either side come from the neighbouring lanes' registers; lane 0 and lane 63, whose
// neighbours are another tile's, fetch theirs, or take 0 outside the window.  All four rows' loads are issued before the
// sRGB tables go to LDS.  A row's group whose sixteen bytes are all zero costs nothing more.  The destination is loaded
// only where some pixel of the group is touched without being covered on all three channels, and stored only where one
// is touched, as one 16-byte access where the flags allow it and the store covers all four pixels.
template <int SRGB>
__global__ __launch_bounds__(64 * LAYER_WAVES) void layer_lcd_kernel(LcdArgs a)
{
    constexpr uint32_t ROWS = LAYER_TILE_H / LAYER_WAVES, GROUP = (1u << LAYER_LANE_PX) - 1u, SUB = 3 * LAYER_LANE_PX;
    const LcdTile t = a.tiles[blockIdx.x];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t gx = t.x + LAYER_LANE_PX * lane, y = t.y + ROWS * wave;
    uint32_t valid = 0;                                        // bit i: column gx + i belongs to the blit
#pragma unroll
    for (uint32_t i = 0; i < LAYER_LANE_PX; ++i) valid |= (gx + i >= t.x0 && gx + i < t.x1) ? 1u << i : 0u;
    const bool dvec = valid == GROUP && (t.vec & LAYER_DST_VEC);

    // which of the lane's elements lie in the window: a mask per dword; e0 + SUB stays far below 2^31
    const int32_t e0 = t.sq + (int32_t)(SUB * lane), q0 = (int32_t)t.q0, q1 = (int32_t)t.q1;
    uint32_t msk[3] = {0u, 0u, 0u};
#pragma unroll
    for (uint32_t b = 0; b < SUB; ++b) msk[b >> 2] |= (e0 + (int32_t)b >= q0 && e0 + (int32_t)b < q1) ? 0xffu << (8 * (b & 3u)) : 0u;
    const bool some = (msk[0] | msk[1] | msk[2]) != 0u;
    const bool cvec = some && (t.vec & LAYER_SRC_VEC) && e0 >= 0 && (uint64_t)(e0 + (int32_t)SUB) <= a.cov_stride;
    // the taps beyond the wave's ends: bit 0, 1: elements e0 - 2, e0 - 1 (lane 0); bit 2, 3: e0 + 12, e0 + 13 (lane 63)
    uint32_t ends = 0;
    if (lane == 0u) ends = (e0 - 2 >= q0 && e0 - 2 < q1 ? 1u : 0u) | (e0 - 1 >= q0 && e0 - 1 < q1 ? 2u : 0u);
    if (lane == 63u) ends = (e0 + 12 >= q0 && e0 + 12 < q1 ? 4u : 0u) | (e0 + 13 >= q0 && e0 + 13 < q1 ? 8u : 0u);

    uint32_t c[ROWS][3], side[ROWS];                           // side: the fetched taps, left in bits 0 - 15, right in 16 - 31
#pragma unroll
    for (uint32_t r = 0; r < ROWS; ++r) {
        c[r][0] = c[r][1] = c[r][2] = side[r] = 0u;
        if (y + r >= t.y1) continue;                           // below the blit: nothing to store
        const uint8_t *p = a.cov + ((int64_t)((uint64_t)(t.sy + ROWS * wave + r) * a.cov_stride) + (int64_t)e0);
        if (cvec) {
            const uint32_t *pw = reinterpret_cast<const uint32_t *>(p);
            c[r][0] = pw[0] & msk[0]; c[r][1] = pw[1] & msk[1]; c[r][2] = pw[2] & msk[2];
        } else if (some) {
#pragma unroll
            for (uint32_t b = 0; b < SUB; ++b)
                if (msk[b >> 2] >> (8 * (b & 3u)) & 1u) c[r][b >> 2] |= (uint32_t)p[b] << (8 * (b & 3u));
        }
        if (ends & 1u) side[r] |= (uint32_t)p[-2];
        if (ends & 2u) side[r] |= (uint32_t)p[-1] << 8;
        if (ends & 4u) side[r] |= (uint32_t)p[12] << 16;
        if (ends & 8u) side[r] |= (uint32_t)p[13] << 24;
    }

    [[maybe_unused]] const uint16_t *D = nullptr, *K = nullptr;
    if constexpr (SRGB) {
        __shared__ uint4 lds_d[sizeof SRGB_D / 16], lds_k[sizeof SRGB_K / 16];
        for (uint32_t i = threadIdx.x; i < sizeof SRGB_K / 16; i += 64 * LAYER_WAVES)
            lds_k[i] = reinterpret_cast<const uint4 *>(SRGB_K)[i];
        if (threadIdx.x < sizeof SRGB_D / 16) lds_d[threadIdx.x] = reinterpret_cast<const uint4 *>(SRGB_D)[threadIdx.x];
        __syncthreads();
        D = reinterpret_cast<const uint16_t *>(lds_d);
        K = reinterpret_cast<const uint16_t *>(lds_k);
    }
    const uint32_t A = t.rgba >> 24;
    uint32_t cl[3];
#pragma unroll
    for (int b = 0; b < 3; ++b) cl[b] = SRGB ? (uint32_t)D[(t.rgba >> (8 * b)) & 0xffu] : (t.rgba >> (8 * b)) & 0xffu;

    uint32_t *__restrict__ dp = a.dst + ((uint64_t)y * a.dst_stride + gx);
#pragma unroll
    for (uint32_t r = 0; r < ROWS; ++r) {
        // every lane of the wave takes part in the moves, whatever it goes on to do
        const uint32_t up = (uint32_t)__shfl_up((int)c[r][2], 1), dn = (uint32_t)__shfl_down((int)c[r][0], 1);
        const uint32_t left = lane == 0u ? side[r] & 0xffffu : up >> 16, right = lane == 63u ? side[r] >> 16 : dn & 0xffffu;
        // the sixteen bytes e0 - 2 .. e0 + 13
        const uint32_t w[4] = {left | c[r][0] << 16, c[r][0] >> 16 | c[r][1] << 16, c[r][1] >> 16 | c[r][2] << 16, c[r][2] >> 16 | right << 16};
        if (!(w[0] | w[1] | w[2] | w[3])) continue;
        uint32_t f[SUB];
#pragma unroll
        for (uint32_t k = 0; k < SUB; ++k) {
            uint32_t s = 128u;
#pragma unroll
            for (uint32_t i = 0; i < FR_LCD_TAPS; ++i) s += a.w[i] * (w[(k + i) >> 2] >> (8 * ((k + i) & 3u)) & 0xffu);
            f[k] = s >> 8;
        }
        uint32_t al[LAYER_LANE_PX][3], touch = 0, part = 0;    // bit i: some a_b != 0; and not all three 255
#pragma unroll
        for (uint32_t i = 0; i < LAYER_LANE_PX; ++i) {
            uint32_t any = 0, all = 255u;
#pragma unroll
            for (uint32_t b = 0; b < 3; ++b) {
                al[i][b] = (valid >> i & 1u) ? m2(a.bgr ? f[3 * i + 2 - b] : f[3 * i + b], A) : 0u;
                any |= al[i][b];
                all &= al[i][b];
            }
            touch |= any ? 1u << i : 0u;
            part |= any && all != 255u ? 1u << i : 0u;
        }
        if (!touch) continue;
        uint32_t *p = dp + (uint64_t)r * a.dst_stride;
        if (dvec && (part || touch == GROUP)) {
            uint4 v = make_uint4(0u, 0u, 0u, 0u);
            if (part) v = *reinterpret_cast<const uint4 *>(p);
            v.x = over_px_ca<SRGB>(cl, v.x, al[0], D, K);
            v.y = over_px_ca<SRGB>(cl, v.y, al[1], D, K);
            v.z = over_px_ca<SRGB>(cl, v.z, al[2], D, K);
            v.w = over_px_ca<SRGB>(cl, v.w, al[3], D, K);
            *reinterpret_cast<uint4 *>(p) = v;
        } else {
#pragma unroll
            for (uint32_t i = 0; i < LAYER_LANE_PX; ++i) {
                if (!(touch >> i & 1u)) continue;              // (0 too where the column or the row is outside the blit)
                p[i] = over_px_ca<SRGB>(cl, (part >> i & 1u) ? p[i] : 0u, al[i], D, K);
            }
        }
    }
}

hipError_t launch_layer_lcd(bool srgb, uint32_t n_tiles, const LcdArgs &a, hipStream_t stream)
{
    hipLaunchKernelGGL(srgb ? layer_lcd_kernel<1> : layer_lcd_kernel<0>, dim3(n_tiles), dim3(64 * LAYER_WAVES), 0, stream, a);
    return hipGetLastError();
}

}  // namespace fr

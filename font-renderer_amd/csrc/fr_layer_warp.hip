// fr_layer_warp.hip — compositing a premultiplied layer over an image through an affine map, sampled bilinearly in exact
// integers (fr_layer_warp; include/fr_raster.h, DESIGN.md sections 4.15 and 5).  The composite is that of fr_layer_px.hpp;
// the taps are gathered from global memory, lane by lane.
#include "fr_layer_warp.hpp"
#include "fr_layer_px.hpp"
#include "fr_srgb.hpp"

namespace fr {

// one byte (or one 16-bit linear value) through the header's formula: at most 65535 * 65536 + 32768 < 2^32
__device__ __forceinline__ uint32_t bilerp1(uint32_t p00, uint32_t p10, uint32_t p01, uint32_t p11, uint32_t fx, uint32_t fy)
{
    const uint32_t top = p00 * (256u - fx) + p10 * fx, bot = p01 * (256u - fx) + p11 * fx;
    return (top * (256u - fy) + bot * fy + 32768u) >> 16;
}

// the four bytes of a pixel: the horizontal step on two bytes at once (a byte's sum is at most 255 * 256 and stays in its
// 16-bit half), the vertical step byte by byte
__device__ __forceinline__ uint32_t bilerp4(uint32_t p00, uint32_t p10, uint32_t p01, uint32_t p11, uint32_t fx, uint32_t fy)
{
    const uint32_t gx = 256u - fx, gy = 256u - fy;
    const uint32_t t02 = (p00 & M2) * gx + (p10 & M2) * fx, t13 = ((p00 >> 8) & M2) * gx + ((p10 >> 8) & M2) * fx;
    const uint32_t b02 = (p01 & M2) * gx + (p11 & M2) * fx, b13 = ((p01 >> 8) & M2) * gx + ((p11 >> 8) & M2) * fx;
    const uint32_t c0 = ((t02 & 0xffffu) * gy + (b02 & 0xffffu) * fy + 32768u) >> 16, c2 = ((t02 >> 16) * gy + (b02 >> 16) * fy + 32768u) >> 16;
    const uint32_t c1 = ((t13 & 0xffffu) * gy + (b13 & 0xffffu) * fy + 32768u) >> 16, c3 = ((t13 >> 16) * gy + (b13 >> 16) * fy + 32768u) >> 16;
    return c0 | c1 << 8 | c2 << 16 | c3 << 24;
}

// v brought into [lo, hi]
__device__ __forceinline__ uint32_t into(int64_t v, uint32_t lo, uint32_t hi)
{
    return v < (int64_t)lo ? lo : v > (int64_t)hi ? hi : (uint32_t)v;
}

// One workgroup per tile of the table (fr_layer_warp_plan.hpp): lane l of wave w owns the four pixels at columns
// t.x + 4 (l mod 8) .. + 3 of row t.y + 8 w + l div 8, so a wave covers 32 x 8 pixels and its taps a patch of the window
// of about that size under any turn.  U and V are 64-bit: a lane adds its offset to the tile's origin and steps by
// (ux, vx) from pixel to pixel.  A tap inside the window is loaded from its own address and one outside from the nearest
// pixel of the tile's tap box and then replaced by zero, so the sixteen loads of a lane are issued together with no branch
// between them and none leaves the box.  A lane none of whose taps is in the window loads nothing; a group whose samples
// are all zero is neither loaded from the image nor stored, nor is the image loaded where every a' is 255.  A group that
// lies wholly inside the rectangle moves its image pixels as 16 bytes where the tile's flag allows; a group cut by the
// rectangle's left or right edge goes pixel by pixel and touches only pixels of the rectangle.
template <int SRGB, int OPACITY>
__global__ __launch_bounds__(64 * LAYER_WAVES) void layer_warp_kernel(WarpArgs a)
{
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
    constexpr uint32_t GROUP = (1u << LAYER_LANE_PX) - 1u;
    const WarpTile t = a.tiles[blockIdx.x];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t dx = LAYER_LANE_PX * (lane & 7u), dy = 8u * wave + (lane >> 3);
    const uint32_t gx = t.x + dx, y = t.y + dy, o = t.ov & 0xffu;
    uint32_t valid = 0;                                        // bit i: column gx + i belongs to the rectangle
#pragma unroll
    for (uint32_t i = 0; i < LAYER_LANE_PX; ++i) valid |= (gx + i >= t.x0 && gx + i < t.x1) ? 1u << i : 0u;
    if (!valid || y >= t.y1) return;

    // the taps of the four pixels: which of them are in the window (bit 0: (i, j), 1: (i+1, j), 2: (i, j+1), 3: (i+1, j+1)),
    // and the columns and rows to load from, kept inside the tap box
    const int64_t U0 = t.U + (int64_t)dx * t.ux + (int64_t)dy * t.uy - WARP_HALF, V0 = t.V + (int64_t)dx * t.vx + (int64_t)dy * t.vy - WARP_HALF;
    uint32_t in[LAYER_LANE_PX], fx[LAYER_LANE_PX], fy[LAYER_LANE_PX], c0[LAYER_LANE_PX], c1[LAYER_LANE_PX], r0[LAYER_LANE_PX], r1[LAYER_LANE_PX];
#pragma unroll
    for (uint32_t i = 0; i < LAYER_LANE_PX; ++i) {
        const int64_t P = U0 + (int64_t)i * t.ux, Q = V0 + (int64_t)i * t.vx;
        const int64_t ci = P >> 16, cj = Q >> 16;
        fx[i] = (uint32_t)(P >> 8) & 0xffu;
        fy[i] = (uint32_t)(Q >> 8) & 0xffu;
        const bool i0 = (uint64_t)ci < t.ww, i1 = (uint64_t)(ci + 1) < t.ww, j0 = (uint64_t)cj < t.wh, j1 = (uint64_t)(cj + 1) < t.wh;
        in[i] = (valid >> i & 1u) ? (i0 && j0 ? 1u : 0u) | (i1 && j0 ? 2u : 0u) | (i0 && j1 ? 4u : 0u) | (i1 && j1 ? 8u : 0u) : 0u;
        c0[i] = into(ci, t.i0, t.i1);
        c1[i] = into(ci + 1, t.i0, t.i1);
        r0[i] = into(cj, t.j0, t.j1);
        r1[i] = into(cj + 1, t.j0, t.j1);
    }
    if (!(in[0] | in[1] | in[2] | in[3])) return;
    const uint32_t *win = a.src + ((uint64_t)t.wy * a.src_stride + t.wx);
    uint32_t p[LAYER_LANE_PX][4];
#pragma unroll
    for (uint32_t i = 0; i < LAYER_LANE_PX; ++i) {
        const uint32_t *top = win + (uint64_t)r0[i] * a.src_stride, *bot = win + (uint64_t)r1[i] * a.src_stride;
        p[i][0] = top[c0[i]];
        p[i][1] = top[c1[i]];
        p[i][2] = bot[c0[i]];
        p[i][3] = bot[c1[i]];
    }
    // the samples: s, the four bytes (with FR_LAYER_SRGB only its alpha is used), and S, the linear colour values
    uint32_t s[LAYER_LANE_PX];
    [[maybe_unused]] uint32_t S[LAYER_LANE_PX][3];
    uint32_t live = 0, opaque = 1;
#pragma unroll
    for (uint32_t i = 0; i < LAYER_LANE_PX; ++i) {
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k) p[i][k] = (in[i] >> k & 1u) ? p[i][k] : 0u;
        uint32_t any;
        if constexpr (!SRGB) {
            any = s[i] = bilerp4(p[i][0], p[i][1], p[i][2], p[i][3], fx[i], fy[i]);
        } else {
            s[i] = bilerp1(p[i][0] >> 24, p[i][1] >> 24, p[i][2] >> 24, p[i][3] >> 24, fx[i], fy[i]) << 24;
            any = s[i];
#pragma unroll
            for (uint32_t c = 0; c < 3; ++c) {
                S[i][c] = bilerp1(D[(p[i][0] >> (8 * c)) & 0xffu], D[(p[i][1] >> (8 * c)) & 0xffu], D[(p[i][2] >> (8 * c)) & 0xffu],
                                  D[(p[i][3] >> (8 * c)) & 0xffu], fx[i], fy[i]);
                any |= S[i][c];
            }
        }
        live |= any ? 1u << i : 0u;                            // (a sample of zero gives the pixel back)
        opaque &= alpha_of<OPACITY>(s[i], o) == 255u ? 1u : 0u;
    }
    if (!live) return;
    const auto px = [&](uint32_t i, uint32_t d) {
        if constexpr (!SRGB) return over_px<0, OPACITY>(s[i], d, o, D, K);
        else return over_px_lin<OPACITY>(s[i] >> 24, S[i], d, o, D, K);
    };
    uint32_t *__restrict__ dp = a.dst + ((uint64_t)y * a.dst_stride + gx);
    if (valid == GROUP && (t.ov & LAYER_DST_VEC)) {
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (!opaque) v = *reinterpret_cast<const uint4 *>(dp);
        v.x = px(0, v.x);
        v.y = px(1, v.y);
        v.z = px(2, v.z);
        v.w = px(3, v.w);
        *reinterpret_cast<uint4 *>(dp) = v;
    } else {
#pragma unroll
        for (uint32_t i = 0; i < LAYER_LANE_PX; ++i) {
            if (!(live >> i & 1u)) continue;                   // (not live too where the column is outside the rectangle)
            const uint32_t d = alpha_of<OPACITY>(s[i], o) == 255u ? 0u : dp[i];
            dp[i] = px(i, d);
        }
    }
}

hipError_t launch_layer_warp(bool srgb, bool opacity, uint32_t n_tiles, const WarpArgs &a, hipStream_t stream)
{
    void (*const kern[2][2])(WarpArgs) = {{layer_warp_kernel<0, 0>, layer_warp_kernel<0, 1>}, {layer_warp_kernel<1, 0>, layer_warp_kernel<1, 1>}};
    hipLaunchKernelGGL(kern[srgb][opacity], dim3(n_tiles), dim3(64 * LAYER_WAVES), 0, stream, a);
    return hipGetLastError();
}

}  // namespace fr

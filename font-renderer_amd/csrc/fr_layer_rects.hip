// fr_layer_rects.hip — anti-aliased rectangles composited over an image (fr_layer_rects; include/fr_raster.h; DESIGN.md
// sections 4.10 and 5).  Bandwidth-bound like fr_layer.hip, whose pixel arithmetic it shares (fr_layer_px.hpp): a rectangle's
// pixel is the layer pixel (R, G, B, 255) at opacity a = m(k, A).
#include "fr_layer_rects.hpp"
#include "fr_layer_px.hpp"
#include "fr_srgb.hpp"

namespace fr {

namespace {

// the 1/64 pixels of [lo, hi) inside the pixel that starts at 64 p: 0 .. 64.  p < 2^25 and the edges are at most 2^31 - 1, so
// both terms fit 32 bits and their difference an int32.
__device__ __forceinline__ uint32_t overlap64(uint32_t lo, uint32_t hi, uint32_t p)
{
    return (uint32_t)max(0, (int32_t)(min(hi, 64u * p + 64u) - max(lo, 64u * p)));
}

}  // namespace

// One workgroup per tile of the table (fr_layer_rects_plan.hpp), with layer_over_kernel's ownership: lane l of every wave
// owns the four pixels at columns t.x + 4 l .. + 3 of the rows t.y + 4 w .. + 3 of its wave w, and keeps all sixteen in
// registers while it walks the tile's rectangles in order.  The walk is uniform across the workgroup, so a rectangle's
// record arrives through scalar loads, whatever the list's length.  A pixel is loaded when the first rectangle that needs
// its bytes comes by (0 < a < 255; an opaque pixel needs none), and stored once at the end if some rectangle changed it.
// A row's group moves as one 16-byte access where the rows are 16-byte aligned and all four pixels lie inside a bounding
// box; else pixel by pixel, only pixels inside one.  `have`, `dirty`: bit 4 r + i for pixel i of row r.
template <int SRGB>
__global__ __launch_bounds__(64 * LAYER_WAVES) void layer_rects_kernel(RectsArgs a)
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
    const RectTile t = a.tiles[blockIdx.x];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    constexpr uint32_t ROWS = LAYER_TILE_H / LAYER_WAVES, GROUP = (1u << LAYER_LANE_PX) - 1u;
    const uint32_t gx = t.x + LAYER_LANE_PX * lane, y = t.y + ROWS * wave;
    uint32_t *__restrict__ dp = a.dst + ((uint64_t)y * a.dst_stride + gx);

    uint32_t px[ROWS][LAYER_LANE_PX] = {};
    uint32_t have = 0, dirty = 0;
    for (uint32_t j = 0; j < t.count; ++j) {
        const RectRec c = a.recs[a.list[t.first + j]];
        uint32_t cx[LAYER_LANE_PX], in_x = 0;
#pragma unroll
        for (uint32_t i = 0; i < LAYER_LANE_PX; ++i) {
            cx[i] = overlap64(c.x0, c.x1, gx + i);
            in_x |= cx[i] ? 1u << i : 0u;
        }
        if (!in_x) continue;
        const uint32_t s = c.rgba | 0xff000000u, A = c.rgba >> 24;
#pragma unroll
        for (uint32_t r = 0; r < ROWS; ++r) {
            const uint32_t cy = overlap64(c.y0, c.y1, y + r);
            if (!cy) continue;
            uint32_t al[LAYER_LANE_PX], touch = 0, part = 0;      // bit i: a != 0; 0 < a < 255
#pragma unroll
            for (uint32_t i = 0; i < LAYER_LANE_PX; ++i) {
                al[i] = m2((255u * cx[i] * cy + 2048u) >> 12, A);
                touch |= al[i] ? 1u << i : 0u;
                part |= al[i] && al[i] != 255u ? 1u << i : 0u;
            }
            if (!touch) continue;
            const uint32_t need = part & ~(have >> (LAYER_LANE_PX * r));   // the pixels whose bytes are wanted and not here yet
            uint32_t *p = dp + (uint64_t)r * a.dst_stride;
            if (need) {
                if (a.dst_vec && in_x == GROUP && !(have >> (LAYER_LANE_PX * r) & GROUP)) {
                    const uint4 v = *reinterpret_cast<const uint4 *>(p);
                    px[r][0] = v.x; px[r][1] = v.y; px[r][2] = v.z; px[r][3] = v.w;
                    have |= GROUP << (LAYER_LANE_PX * r);
                } else {
#pragma unroll
                    for (uint32_t i = 0; i < LAYER_LANE_PX; ++i)
                        if (need >> i & 1u) px[r][i] = p[i];
                }
            }
            if (touch == GROUP && !part) {
                // a = 255 on all four, the inside of an opaque rectangle: (R, G, B, 255) in both spaces (m(x, 255) = x,
                // E(D[v]) = v), and no bit of the pixels under it
#pragma unroll
                for (uint32_t i = 0; i < LAYER_LANE_PX; ++i) px[r][i] = s;
            } else {
#pragma unroll
                for (uint32_t i = 0; i < LAYER_LANE_PX; ++i)
                    if (touch >> i & 1u) px[r][i] = over_px<SRGB, 1>(s, px[r][i], al[i], D, K);
            }
            have |= touch << (LAYER_LANE_PX * r);
            dirty |= touch << (LAYER_LANE_PX * r);
        }
    }
#pragma unroll
    for (uint32_t r = 0; r < ROWS; ++r) {
        const uint32_t d = dirty >> (LAYER_LANE_PX * r) & GROUP;
        if (!d) continue;
        uint32_t *p = dp + (uint64_t)r * a.dst_stride;
        if (a.dst_vec && (have >> (LAYER_LANE_PX * r) & GROUP) == GROUP) {
            *reinterpret_cast<uint4 *>(p) = make_uint4(px[r][0], px[r][1], px[r][2], px[r][3]);
        } else {
#pragma unroll
            for (uint32_t i = 0; i < LAYER_LANE_PX; ++i)
                if (d >> i & 1u) p[i] = px[r][i];
        }
    }
}

hipError_t launch_layer_rects(bool srgb, uint32_t n_tiles, const RectsArgs &a, hipStream_t stream)
{
    hipLaunchKernelGGL(srgb ? layer_rects_kernel<1> : layer_rects_kernel<0>, dim3(n_tiles), dim3(64 * LAYER_WAVES), 0, stream, a);
    return hipGetLastError();
}

}  // namespace fr

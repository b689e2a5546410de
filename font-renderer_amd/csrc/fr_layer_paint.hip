// fr_layer_paint.hip — a linear or radial gradient composited over an image through a layer's alpha (fr_layer_paint;
// include/fr_raster.h; DESIGN.md sections 4.11 and 5).  Bandwidth-bound like fr_layer.hip and fr_layer_rects.hip, whose
// pixel arithmetic it shares (fr_layer_px.hpp): a painted pixel is the layer pixel (R, G, B, 255) of the gradient's table
// at opacity a = m(cov, A).
#include "fr_layer_paint.hpp"
#include "fr_layer_px.hpp"
#include "fr_srgb.hpp"

namespace fr {

namespace {

// t -> u in 0 .. 65535 (the header's three spreads; `&` is the floor mod of a two's complement t)
__device__ __forceinline__ uint32_t spread_u(int64_t t, uint32_t spread)
{
    if (spread == FR_SPREAD_PAD) return (uint32_t)(t < 0 ? 0 : t > 65535 ? 65535 : t);
    const uint32_t v = (uint32_t)t & 131071u;
    if (spread == FR_SPREAD_REPEAT) return v & 65535u;
    return v < 65536u ? v : 131071u - v;
}

// t of the radial gradient at (ddx, ddy) from the centre, |ddx|, |ddy| < 2^27: s = isqrt((ddx^2 + ddy^2) 256), then
// floor(s R / 2^48) from the 128-bit product.  The binary64 root of the binary64 value of v < 2^63 lies within 2^-20 of
// the exact root, so its integer part is the floor root or one beside it: one step down and one step up settle it.
// (A lane outside the rectangle may come with larger values; its arithmetic wraps and its result is not used.)
__device__ __forceinline__ int64_t radial_t(int64_t ddx, int64_t ddy, uint64_t R)
{
    const uint64_t v = ((uint64_t)(ddx * ddx) + (uint64_t)(ddy * ddy)) << 8;
    uint64_t s = (uint64_t)sqrt((double)v);
    s -= s * s > v ? 1u : 0u;
    s += (s + 1) * (s + 1) <= v ? 1u : 0u;
    return (int64_t)(__umul64hi(s, R) << 16 | (s * R) >> 48);
}

}  // namespace

// One workgroup per tile of the clipped rectangle, tile blockIdx.x % tiles_x of tile row blockIdx.x / tiles_x, with
// layer_over_kernel's ownership: lane l of every wave owns the four pixels at columns x + 4 l .. + 3 of the rows y + 4 w
// .. + 3 of its wave w.  The four rows' layer loads are issued first, then the colour table (and the sRGB tables) go into
// LDS.  A row's group whose coverage is all zero costs nothing more: an empty tile of a text layer is the layer read
// alone.  Else t comes from one 64-bit multiply-add per lane, an add per row and an add per pixel (linear), or from the
// exact integer root (radial); the destination is loaded only where some pixel of the group has 0 < a < 255 and stored
// only where some pixel has a != 0, as one 16-byte access where the flags allow it and the store covers all four pixels.
template <int SRGB, int KIND, int SRC>
__global__ __launch_bounds__(64 * LAYER_WAVES) void layer_paint_kernel(PaintArgs a)
{
    constexpr uint32_t ROWS = LAYER_TILE_H / LAYER_WAVES, GROUP = (1u << LAYER_LANE_PX) - 1u;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t bx = blockIdx.x % a.tiles_x, by = blockIdx.x / a.tiles_x;
    const uint32_t gx = a.tx0 + LAYER_TILE_W * bx + LAYER_LANE_PX * lane, row0 = LAYER_TILE_H * by + ROWS * wave, y = a.y0 + row0;
    uint32_t valid = 0;                                        // bit i: column gx + i belongs to the rectangle
#pragma unroll
    for (uint32_t i = 0; i < LAYER_LANE_PX; ++i) valid |= (gx + i >= a.x0 && gx + i < a.x1) ? 1u << i : 0u;
    const bool whole = valid == GROUP;
    const bool svec = SRC && whole && (a.vec & LAYER_SRC_VEC), dvec = whole && (a.vec & LAYER_DST_VEC);

    uint32_t cov[ROWS][LAYER_LANE_PX];
#pragma unroll
    for (uint32_t r = 0; r < ROWS; ++r) {
        if (y + r >= a.y1) {
#pragma unroll
            for (uint32_t i = 0; i < LAYER_LANE_PX; ++i) cov[r][i] = 0u;     // below the rectangle
        } else if constexpr (!SRC) {
#pragma unroll
            for (uint32_t i = 0; i < LAYER_LANE_PX; ++i) cov[r][i] = (valid >> i & 1u) ? 255u : 0u;
        } else {
            const uint32_t *p = a.src + ((uint64_t)(a.sy + row0 + r) * a.src_stride + (int64_t)(a.sx0 + (int32_t)(gx - a.tx0)));
            if (svec) {
                const uint4 v = *reinterpret_cast<const uint4 *>(p);
                cov[r][0] = v.x >> 24; cov[r][1] = v.y >> 24; cov[r][2] = v.z >> 24; cov[r][3] = v.w >> 24;
            } else {
#pragma unroll
                for (uint32_t i = 0; i < LAYER_LANE_PX; ++i) cov[r][i] = (valid >> i & 1u) ? p[i] >> 24 : 0u;
            }
        }
    }

    __shared__ uint4 lds_g[PAINT_TABLE / 4];
    static_assert(PAINT_TABLE / 4 == 64 * LAYER_WAVES, "one unit of the colour table per thread");
    lds_g[threadIdx.x] = reinterpret_cast<const uint4 *>(a.table)[threadIdx.x];
    [[maybe_unused]] const uint16_t *D = nullptr, *K = nullptr;
    if constexpr (SRGB) {
        __shared__ uint4 lds_d[sizeof SRGB_D / 16], lds_k[sizeof SRGB_K / 16];
        for (uint32_t i = threadIdx.x; i < sizeof SRGB_K / 16; i += 64 * LAYER_WAVES)
            lds_k[i] = reinterpret_cast<const uint4 *>(SRGB_K)[i];
        if (threadIdx.x < sizeof SRGB_D / 16) lds_d[threadIdx.x] = reinterpret_cast<const uint4 *>(SRGB_D)[threadIdx.x];
        D = reinterpret_cast<const uint16_t *>(lds_d);
        K = reinterpret_cast<const uint16_t *>(lds_k);
    }
    __syncthreads();
    const uint32_t *G = reinterpret_cast<const uint32_t *>(lds_g);

    // linear: t 2^16 of pixel (gx, y); radial: the pixel's distance from the centre in 1/64 pixel
    const int64_t lin = KIND ? 0 : a.c[0] + (int64_t)gx * a.c[1] + (int64_t)y * a.c[2];
    const int64_t ddx = 64 * (int64_t)gx + 32 - a.c[0], ddy = 64 * (int64_t)y + 32 - a.c[1];
    uint32_t *__restrict__ dp = a.dst + ((uint64_t)y * a.dst_stride + gx);
#pragma unroll
    for (uint32_t r = 0; r < ROWS; ++r) {
        if (!(cov[r][0] | cov[r][1] | cov[r][2] | cov[r][3])) continue;
        uint32_t s[LAYER_LANE_PX], al[LAYER_LANE_PX], touch = 0, part = 0;     // bit i: a != 0; 0 < a < 255
#pragma unroll
        for (uint32_t i = 0; i < LAYER_LANE_PX; ++i) {
            const int64_t t = KIND ? radial_t(ddx + 64 * (int64_t)i, ddy + 64 * (int64_t)r, (uint64_t)a.c[2])
                                   : (lin + (int64_t)r * a.c[2] + (int64_t)i * a.c[1]) >> 16;
            const uint32_t g = G[spread_u(t, a.spread) >> 6];
            s[i] = g | 0xff000000u;
            al[i] = m2(cov[r][i], g >> 24);
            touch |= al[i] ? 1u << i : 0u;
            part |= al[i] && al[i] != 255u ? 1u << i : 0u;
        }
        if (!touch) continue;
        uint32_t *p = dp + (uint64_t)r * a.dst_stride;
        if (dvec && (part || touch == GROUP)) {
            uint4 v = make_uint4(s[0], s[1], s[2], s[3]);
            if (part) {
                // a = 0 gives the pixel back; a = 255 takes no bit of it
                v = *reinterpret_cast<const uint4 *>(p);
                v.x = over_px<SRGB, 1>(s[0], v.x, al[0], D, K);
                v.y = over_px<SRGB, 1>(s[1], v.y, al[1], D, K);
                v.z = over_px<SRGB, 1>(s[2], v.z, al[2], D, K);
                v.w = over_px<SRGB, 1>(s[3], v.w, al[3], D, K);
            }
            // else a = 255 on all four, opaque stops under solid coverage: (R, G, B, 255) in both spaces (m(x, 255) = x,
            // E(D[v]) = v), without the blend
            *reinterpret_cast<uint4 *>(p) = v;
        } else {
#pragma unroll
            for (uint32_t i = 0; i < LAYER_LANE_PX; ++i) {
                if (!(touch >> i & 1u)) continue;                          // (0 too where the column or the row is outside the rectangle)
                p[i] = (part >> i & 1u) ? over_px<SRGB, 1>(s[i], p[i], al[i], D, K) : s[i];    // (a = 255: the colour itself)
            }
        }
    }
}

hipError_t launch_layer_paint(bool srgb, bool radial, uint32_t n_tiles, const PaintArgs &a, hipStream_t stream)
{
    void (*const kern[2][2][2])(PaintArgs) = {{{layer_paint_kernel<0, 0, 0>, layer_paint_kernel<0, 0, 1>}, {layer_paint_kernel<0, 1, 0>, layer_paint_kernel<0, 1, 1>}},
                                              {{layer_paint_kernel<1, 0, 0>, layer_paint_kernel<1, 0, 1>}, {layer_paint_kernel<1, 1, 0>, layer_paint_kernel<1, 1, 1>}}};
    hipLaunchKernelGGL(kern[srgb][radial][a.src != nullptr], dim3(n_tiles), dim3(64 * LAYER_WAVES), 0, stream, a);
    return hipGetLastError();
}

}  // namespace fr

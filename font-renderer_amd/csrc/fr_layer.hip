// fr_layer.hip — compositing a finished premultiplied layer over an image (fr_layer_over), and the device twin of
// fr_rgba_unpremultiply (include/fr_raster.h; DESIGN.md sections 4.8 and 5).  Both kernels are bandwidth-bound: the
// arithmetic is that of the text plans' colour body (fr_text_colour.hpp), per pixel instead of per sample.
#include "fr_layer.hpp"
#include "fr_layer_px.hpp"
#include "fr_srgb.hpp"

namespace fr {

// One workgroup per tile of the table (fr_layer_plan.hpp).  Lane l of every wave owns the four pixels at columns
// t.x + 4 l .. + 3; wave w the rows t.y + 4 w .. + 3.  A group that lies wholly inside the blit moves as one 16-byte access
// where the tile's flags allow it; a group cut by the blit's left or right edge, and every group of a tile without the
// flag, goes pixel by pixel and touches only pixels of the blit.  The four rows' layer loads are issued before anything
// depends on them.  A group whose layer pixels are all zero is not stored (4 bytes per pixel of traffic), and its
// destination not loaded; nor is the destination loaded where every a' is 255 (8 bytes per pixel).
template <int SRGB, int OPACITY>
__global__ __launch_bounds__(64 * LAYER_WAVES) void layer_over_kernel(LayerArgs a)
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
    const LayerTile t = a.tiles[blockIdx.x];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t gx = t.x + LAYER_LANE_PX * lane, o = t.ov & 0xffu;
    uint32_t valid = 0;                                        // bit i: column gx + i belongs to the blit
#pragma unroll
    for (uint32_t i = 0; i < LAYER_LANE_PX; ++i) valid |= (gx + i >= t.x0 && gx + i < t.x1) ? 1u << i : 0u;
    if (!valid) return;
    const bool whole = valid == (1u << LAYER_LANE_PX) - 1u;
    const bool svec = whole && (t.ov & LAYER_SRC_VEC), dvec = whole && (t.ov & LAYER_DST_VEC);
    constexpr uint32_t ROWS = LAYER_TILE_H / LAYER_WAVES;
    const uint32_t y = t.y + ROWS * wave;
    const uint32_t *__restrict__ sp = a.src + ((uint64_t)(t.sy + ROWS * wave) * a.src_stride + (int64_t)(t.sx + (int32_t)(LAYER_LANE_PX * lane)));
    uint32_t *__restrict__ dp = a.dst + ((uint64_t)y * a.dst_stride + gx);

    uint32_t s[ROWS][LAYER_LANE_PX];
#pragma unroll
    for (uint32_t r = 0; r < ROWS; ++r) {
        const uint32_t *p = sp + (uint64_t)r * a.src_stride;
        if (y + r >= t.y1) {
#pragma unroll
            for (uint32_t i = 0; i < LAYER_LANE_PX; ++i) s[r][i] = 0u;     // below the blit: nothing to store
        } else if (svec) {
            const uint4 v = *reinterpret_cast<const uint4 *>(p);
            s[r][0] = v.x; s[r][1] = v.y; s[r][2] = v.z; s[r][3] = v.w;
        } else {
#pragma unroll
            for (uint32_t i = 0; i < LAYER_LANE_PX; ++i) s[r][i] = (valid >> i & 1u) ? p[i] : 0u;
        }
    }
#pragma unroll
    for (uint32_t r = 0; r < ROWS; ++r) {
        uint32_t *p = dp + (uint64_t)r * a.dst_stride;
        uint32_t any = 0, opaque = 1;
#pragma unroll
        for (uint32_t i = 0; i < LAYER_LANE_PX; ++i) {
            any |= s[r][i];
            opaque &= alpha_of<OPACITY>(s[r][i], o) == 255u ? 1u : 0u;
        }
        if (!any) continue;
        if (dvec) {
            uint4 v = make_uint4(0u, 0u, 0u, 0u);
            if (!opaque) v = *reinterpret_cast<const uint4 *>(p);
            v.x = over_px<SRGB, OPACITY>(s[r][0], v.x, o, D, K);
            v.y = over_px<SRGB, OPACITY>(s[r][1], v.y, o, D, K);
            v.z = over_px<SRGB, OPACITY>(s[r][2], v.z, o, D, K);
            v.w = over_px<SRGB, OPACITY>(s[r][3], v.w, o, D, K);
            *reinterpret_cast<uint4 *>(p) = v;
        } else {
#pragma unroll
            for (uint32_t i = 0; i < LAYER_LANE_PX; ++i) {
                if (!s[r][i]) continue;                        // (0 too where the column or the row is outside the blit)
                const uint32_t d = alpha_of<OPACITY>(s[r][i], o) == 255u ? 0u : p[i];
                p[i] = over_px<SRGB, OPACITY>(s[r][i], d, o, D, K);
            }
        }
    }
}

// A call's tables from the pinned staging into the DevBuf the composite reads, in the composite's own queue: a copy
// engine's hand-over before and after a 64 KiB copy costs more than the composite of a 3840 x 2160 frame.
__global__ __launch_bounds__(256) void layer_table_kernel(const uint4 *__restrict__ from, uint4 *__restrict__ to, uint32_t n)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < n) to[i] = from[i];
}

hipError_t launch_layer_table(const uint4 *staged, uint4 *table, uint32_t n, hipStream_t stream)
{
    hipLaunchKernelGGL(layer_table_kernel, dim3((n + 255u) / 256u), dim3(256), 0, stream, staged, table, n);
    return hipGetLastError();
}

hipError_t launch_layer_over(bool srgb, bool opacity, uint32_t n_tiles, const LayerArgs &a, hipStream_t stream)
{
    void (*const kern[2][2])(LayerArgs) = {{layer_over_kernel<0, 0>, layer_over_kernel<0, 1>}, {layer_over_kernel<1, 0>, layer_over_kernel<1, 1>}};
    hipLaunchKernelGGL(kern[srgb][opacity], dim3(n_tiles), dim3(64 * LAYER_WAVES), 0, stream, a);
    return hipGetLastError();
}

// ---- fr_layer_unpremultiply -------------------------------------------------------------------------------------------
namespace {

// (255 x + a div 2) div a for x <= 65535: the numerator n is below 2^24, and with M = ceil(2^36 / a) the product n M is
// below 2^61 and (n M) >> 36 = n div a exactly, because n (M a - 2^36) < 2^24 * 255 < 2^36.
struct Recip36 {
    uint64_t m[256];
};
constexpr Recip36 make_recip36()
{
    Recip36 t{};
    for (uint32_t a = 1; a < 256; ++a) t.m[a] = (((uint64_t)1 << 36) + a - 1) / a;
    return t;
}
__constant__ Recip36 RECIP36 = make_recip36();

}  // namespace

// One pixel per lane: a workgroup takes LAYER_TILE_W columns by LAYER_TILE_H rows of the window, row by row.  The three
// cases of fr_rgba_unpremultiply; a pixel that comes out as it went in (alpha 255, or already straight) is not stored.
template <int SRGB>
__global__ __launch_bounds__(LAYER_TILE_W) void layer_unpremultiply_kernel(uint32_t *rgba, uint64_t stride, uint32_t w, uint32_t h, uint32_t tiles_x)
{
    [[maybe_unused]] const uint16_t *D = nullptr, *K = nullptr;
    if constexpr (SRGB) {
        __shared__ uint4 lds_d[sizeof SRGB_D / 16], lds_k[sizeof SRGB_K / 16];
        for (uint32_t i = threadIdx.x; i < sizeof SRGB_K / 16; i += LAYER_TILE_W)
            lds_k[i] = reinterpret_cast<const uint4 *>(SRGB_K)[i];
        if (threadIdx.x < sizeof SRGB_D / 16) lds_d[threadIdx.x] = reinterpret_cast<const uint4 *>(SRGB_D)[threadIdx.x];
        __syncthreads();
        D = reinterpret_cast<const uint16_t *>(lds_d);
        K = reinterpret_cast<const uint16_t *>(lds_k);
    }
    const uint32_t x = (blockIdx.x % tiles_x) * LAYER_TILE_W + threadIdx.x, y0 = (blockIdx.x / tiles_x) * LAYER_TILE_H;
    if (x >= w) return;
    for (uint32_t y = y0; y < y0 + LAYER_TILE_H && y < h; ++y) {
        uint32_t *p = rgba + ((uint64_t)y * stride + x);
        const uint32_t v = *p, al = v >> 24;
        uint32_t out = 0u;
        if (al == 255u) continue;
        if (al != 0u) {
            const uint64_t M = RECIP36.m[al];
            out = v & 0xff000000u;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const uint32_t b = (v >> (8 * c)) & 0xffu;
                const uint32_t q = (uint32_t)(((uint64_t)(255u * (SRGB ? (uint32_t)D[b] : b) + al / 2u) * M) >> 36);
                out |= (SRGB ? srgb_encode(K, min(65535u, q)) : min(255u, q)) << (8 * c);
            }
        }
        if (out != v) *p = out;
    }
}

hipError_t launch_layer_unpremultiply(bool srgb, uint32_t *rgba, uint64_t stride, uint32_t w, uint32_t h, hipStream_t stream)
{
    const uint32_t tiles_x = (w + LAYER_TILE_W - 1) / LAYER_TILE_W, tiles_y = (h + LAYER_TILE_H - 1) / LAYER_TILE_H;
    hipLaunchKernelGGL(srgb ? layer_unpremultiply_kernel<1> : layer_unpremultiply_kernel<0>, dim3(tiles_x * tiles_y), dim3(LAYER_TILE_W), 0, stream,
                       rgba, stride, w, h, tiles_x);
    return hipGetLastError();
}

}  // namespace fr

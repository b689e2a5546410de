// fr_layer_blend.hip — a finished premultiplied layer blended into an image in one of nine separable modes (fr_layer_blend:
// include/fr_raster.h; DESIGN.md sections 4.16 and 5).  The tile walk is layer_over_kernel's (fr_layer.hip); the pixel is
// blend_px (fr_layer_px.hpp).
#include "fr_layer_blend.hpp"
#include "fr_layer_px.hpp"
#include "fr_srgb.hpp"

#include <utility>

namespace fr {

// One workgroup per tile of fr_layer_plan's table, as layer_over_kernel walks it: lane l of every wave owns the four pixels
// at columns t.x + 4 l .. + 3; wave w the rows t.y + 4 w .. + 3.  A group that lies wholly inside the blit moves as one
// 16-byte access where the tile's flags allow it; a group cut by the blit's left or right edge, and every group of a tile
// without the flag, goes pixel by pixel and touches only pixels of the blit.  The four rows' layer loads are issued before
// anything depends on them.  A group whose layer pixels are all zero is neither loaded from the image nor stored (4 bytes
// per pixel of traffic); every other group moves 12 bytes per pixel, because a blend needs the destination under an
// opaque layer pixel too.
template <int SRGB, uint32_t MODE, int OPACITY>
__global__ __launch_bounds__(64 * LAYER_WAVES) void layer_blend_kernel(LayerArgs a)
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
        if (!(s[r][0] | s[r][1] | s[r][2] | s[r][3])) continue;
        if (dvec) {
            uint4 v = *reinterpret_cast<const uint4 *>(p);
            v.x = blend_px<SRGB, MODE, OPACITY>(s[r][0], v.x, o, D, K);
            v.y = blend_px<SRGB, MODE, OPACITY>(s[r][1], v.y, o, D, K);
            v.z = blend_px<SRGB, MODE, OPACITY>(s[r][2], v.z, o, D, K);
            v.w = blend_px<SRGB, MODE, OPACITY>(s[r][3], v.w, o, D, K);
            *reinterpret_cast<uint4 *>(p) = v;
        } else {
#pragma unroll
            for (uint32_t i = 0; i < LAYER_LANE_PX; ++i) {
                if (!s[r][i]) continue;                        // (0 too where the column or the row is outside the blit)
                p[i] = blend_px<SRGB, MODE, OPACITY>(s[r][i], p[i], o, D, K);
            }
        }
    }
}

namespace {

using BlendKernel = void (*)(LayerArgs);

template <int SRGB, int OPACITY, uint32_t... MODE>
constexpr void blend_kernels(BlendKernel (&to)[FR_BLEND_MODES], std::integer_sequence<uint32_t, MODE...>)
{
    ((to[MODE] = layer_blend_kernel<SRGB, MODE, OPACITY>), ...);
}

struct BlendTable {
    BlendKernel k[2][2][FR_BLEND_MODES];                       // [srgb][opacity][mode]
    BlendTable()
    {
        constexpr auto modes = std::make_integer_sequence<uint32_t, FR_BLEND_MODES>{};
        blend_kernels<0, 0>(k[0][0], modes);
        blend_kernels<0, 1>(k[0][1], modes);
        blend_kernels<1, 0>(k[1][0], modes);
        blend_kernels<1, 1>(k[1][1], modes);
    }
};

}  // namespace

hipError_t launch_layer_blend(bool srgb, uint32_t mode, bool opacity, uint32_t n_tiles, const LayerArgs &a, hipStream_t stream)
{
    static const BlendTable table;
    if (mode >= FR_BLEND_MODES) return hipErrorInvalidValue;
    hipLaunchKernelGGL(table.k[srgb][opacity][mode], dim3(n_tiles), dim3(64 * LAYER_WAVES), 0, stream, a);
    return hipGetLastError();
}

}  // namespace fr

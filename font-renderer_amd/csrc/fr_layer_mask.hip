// fr_layer_mask.hip — compositing a premultiplied layer over an image through a mask, or erasing the image through one
// (fr_layer_mask; include/fr_raster.h, DESIGN.md sections 4.14 and 5).  layer_over_kernel (fr_layer.hip) with an opacity per
// pixel: bandwidth-bound, the arithmetic that of fr_layer_px.hpp.
#include "fr_layer_mask.hpp"
#include "fr_layer_px.hpp"
#include "fr_srgb.hpp"

namespace fr {

// One workgroup per tile of the table (fr_layer_mask_plan.hpp), with layer_over_kernel's ownership: lane l of every wave
// owns the four pixels at columns t.x + 4 l .. + 3, wave w the rows t.y + 4 w .. + 3.  A group that lies wholly inside the
// blit reads its four mask elements as one access (16 bytes of a layer mask, 4 of a plane) and moves its layer and image
// pixels as 16 bytes each where the tile's flags allow; a group cut by the blit's left or right edge, and every group of a
// tile without the flag, goes element by element and touches only elements of the blit.  The four rows' mask and layer
// loads are issued before anything depends on them; t = m(k', o) is taken of two pixels at a time.  A group in which no
// pixel has both t != 0 and a layer pixel != 0 (erase: t != 0) is neither loaded from the image nor stored; nor is the
// image loaded where every a' (erase: every t) is 255.
template <int SRGB, int PLANE, int ERASE>
__global__ __launch_bounds__(64 * LAYER_WAVES) void layer_mask_kernel(MaskArgs a)
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
    constexpr uint32_t ROWS = LAYER_TILE_H / LAYER_WAVES, GROUP = (1u << LAYER_LANE_PX) - 1u;
    const MaskTile t = a.tiles[blockIdx.x];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t gx = t.x + LAYER_LANE_PX * lane, o = t.ov & 0xffu, inv2 = t.invert ? M2 : 0u;
    uint32_t valid = 0;                                        // bit i: column gx + i belongs to the blit
#pragma unroll
    for (uint32_t i = 0; i < LAYER_LANE_PX; ++i) valid |= (gx + i >= t.x0 && gx + i < t.x1) ? 1u << i : 0u;
    if (!valid) return;
    const bool whole = valid == GROUP;
    const bool svec = !ERASE && whole && (t.ov & LAYER_SRC_VEC), dvec = whole && (t.ov & LAYER_DST_VEC), mvec = whole && (t.ov & LAYER_MASK_VEC);
    // the columns of the blit among pixels 0 and 2, and among 1 and 3, as the two channels of an m2
    const uint32_t v02 = (valid & 1u ? 0xffu : 0u) | (valid & 4u ? 0xff0000u : 0u), v13 = (valid & 2u ? 0xffu : 0u) | (valid & 8u ? 0xff0000u : 0u);
    const uint32_t y = t.y + ROWS * wave;
    const int64_t mcol = (int64_t)(t.mx + (int32_t)(LAYER_LANE_PX * lane));

    // What the loads bring is kept as it comes, so that no load waits for another: kv, a layer mask's pixels, or a plane's
    // bytes loaded one by one, or (mvec) its four bytes at once in kv[r][0]; s, the layer's pixels.  All start as 0, which
    // is what an element outside the blit counts as.
    uint32_t kv[ROWS][LAYER_LANE_PX];
    [[maybe_unused]] uint32_t s[ROWS][LAYER_LANE_PX];
    // a group's four mask bytes, element i in byte i
    const auto k_of = [&](uint32_t r) {
        if constexpr (PLANE) return kv[r][0] | kv[r][1] << 8 | kv[r][2] << 16 | kv[r][3] << 24;    // (mvec: all four bytes are in kv[r][0])
        else return kv[r][0] >> 24 | (kv[r][1] >> 24) << 8 | (kv[r][2] >> 24) << 16 | (kv[r][3] & 0xff000000u);
    };
    // t of pixels 0 and 2, and of 1 and 3, from a group's mask bytes; 0 for a column outside the blit
    const auto t02_of = [&](uint32_t kk) { return m2((kk & M2) ^ inv2, o) & v02; };
    const auto t13_of = [&](uint32_t kk) { return m2(((kk >> 8) & M2) ^ inv2, o) & v13; };
    [[maybe_unused]] const auto load_src = [&](uint32_t r) {
        const uint32_t *p = a.src + ((int64_t)((uint64_t)(t.sy + ROWS * wave + r) * a.src_stride) + (int64_t)(t.sx + (int32_t)(LAYER_LANE_PX * lane)));
        if (svec) {
            const uint4 v = *reinterpret_cast<const uint4 *>(p);
            s[r][0] = v.x; s[r][1] = v.y; s[r][2] = v.z; s[r][3] = v.w;
        } else {
#pragma unroll
            for (uint32_t i = 0; i < LAYER_LANE_PX; ++i)
                if (valid >> i & 1u) s[r][i] = p[i];
        }
    };
#pragma unroll
    for (uint32_t r = 0; r < ROWS; ++r) {
#pragma unroll
        for (uint32_t i = 0; i < LAYER_LANE_PX; ++i) kv[r][i] = s[r][i] = 0u;
        // The zeros are in the plane's registers before either of its paths begins: set inside the 4-byte path, those of
        // kv[r][1 .. 3] wait for the byte loads that the other path may have in flight, and with them for every load of
        // the rows before (s_waitcnt vmcnt(1) behind each row's mask load; DESIGN.md 4.14 has what that costs).
        if constexpr (PLANE) asm volatile("" : "+v"(kv[r][0]), "+v"(kv[r][1]), "+v"(kv[r][2]), "+v"(kv[r][3]));
        if (y + r >= t.y1) continue;                           // below the blit: no element is read, nothing is stored
        const int64_t mrow = (int64_t)((uint64_t)(t.my + ROWS * wave + r) * a.mask_stride) + mcol;
        if constexpr (PLANE) {
            const uint8_t *p = static_cast<const uint8_t *>(a.mask) + mrow;
            if (mvec) {
                kv[r][0] = *reinterpret_cast<const uint32_t *>(p);
            } else {
#pragma unroll
                for (uint32_t i = 0; i < LAYER_LANE_PX; ++i)
                    if (valid >> i & 1u) kv[r][i] = p[i];
            }
        } else {
            const uint32_t *p = static_cast<const uint32_t *>(a.mask) + mrow;
            if (mvec) {
                const uint4 v = *reinterpret_cast<const uint4 *>(p);
                kv[r][0] = v.x; kv[r][1] = v.y; kv[r][2] = v.z; kv[r][3] = v.w;
            } else {
#pragma unroll
                for (uint32_t i = 0; i < LAYER_LANE_PX; ++i)
                    if (valid >> i & 1u) kv[r][i] = p[i];
            }
        }
        if constexpr (!ERASE) load_src(r);
    }
    uint32_t *__restrict__ dp = a.dst + ((uint64_t)y * a.dst_stride + gx);
#pragma unroll
    for (uint32_t r = 0; r < ROWS; ++r) {
        if (y + r >= t.y1) continue;
        const uint32_t k = k_of(r), t02 = t02_of(k), t13 = t13_of(k);
        if (!(t02 | t13)) continue;
        const uint32_t tt[LAYER_LANE_PX] = {t02 & 0xffu, t13 & 0xffu, t02 >> 16, t13 >> 16};
        uint32_t *p = dp + (uint64_t)r * a.dst_stride;
        if constexpr (!ERASE) {
            uint32_t live = 0, opaque = 1;
#pragma unroll
            for (uint32_t i = 0; i < LAYER_LANE_PX; ++i) {
                live |= s[r][i] && tt[i] ? 1u << i : 0u;
                opaque &= alpha_of<1>(s[r][i], tt[i]) == 255u ? 1u : 0u;
            }
            if (!live) continue;
            if (dvec) {
                uint4 v = make_uint4(0u, 0u, 0u, 0u);
                if (!opaque) v = *reinterpret_cast<const uint4 *>(p);      // (s == 0 or t == 0 gives the pixel back)
                v.x = over_px<SRGB, 1>(s[r][0], v.x, tt[0], D, K);
                v.y = over_px<SRGB, 1>(s[r][1], v.y, tt[1], D, K);
                v.z = over_px<SRGB, 1>(s[r][2], v.z, tt[2], D, K);
                v.w = over_px<SRGB, 1>(s[r][3], v.w, tt[3], D, K);
                *reinterpret_cast<uint4 *>(p) = v;
            } else {
#pragma unroll
                for (uint32_t i = 0; i < LAYER_LANE_PX; ++i) {
                    if (!(live >> i & 1u)) continue;           // (not live too where the column is outside the blit)
                    const uint32_t d = alpha_of<1>(s[r][i], tt[i]) == 255u ? 0u : p[i];
                    p[i] = over_px<SRGB, 1>(s[r][i], d, tt[i], D, K);
                }
            }
        } else {
            if (dvec) {
                uint4 v = make_uint4(0u, 0u, 0u, 0u);
                if ((t02 & t13) != M2) {                       // else t = 255 on all four: zeros, without the load
                    v = *reinterpret_cast<const uint4 *>(p);
                    v.x = erase_px<SRGB>(v.x, tt[0], D, K);
                    v.y = erase_px<SRGB>(v.y, tt[1], D, K);
                    v.z = erase_px<SRGB>(v.z, tt[2], D, K);
                    v.w = erase_px<SRGB>(v.w, tt[3], D, K);
                }
                *reinterpret_cast<uint4 *>(p) = v;
            } else {
#pragma unroll
                for (uint32_t i = 0; i < LAYER_LANE_PX; ++i) {
                    if (!tt[i]) continue;                      // (0 too where the column is outside the blit)
                    p[i] = tt[i] == 255u ? 0u : erase_px<SRGB>(p[i], tt[i], D, K);
                }
            }
        }
    }
}

hipError_t launch_layer_mask(bool srgb, bool plane, bool erase, uint32_t n_tiles, const MaskArgs &a, hipStream_t stream)
{
    void (*const kern[2][2][2])(MaskArgs) = {{{layer_mask_kernel<0, 0, 0>, layer_mask_kernel<0, 0, 1>}, {layer_mask_kernel<0, 1, 0>, layer_mask_kernel<0, 1, 1>}},
                                             {{layer_mask_kernel<1, 0, 0>, layer_mask_kernel<1, 0, 1>}, {layer_mask_kernel<1, 1, 0>, layer_mask_kernel<1, 1, 1>}}};
    hipLaunchKernelGGL(kern[srgb][plane][erase], dim3(n_tiles), dim3(64 * LAYER_WAVES), 0, stream, a);
    return hipGetLastError();
}

}  // namespace fr

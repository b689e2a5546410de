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
            // cx = (f32(X - ix) + (off(i) - fx)) / scale: off(i) - fx is exact (multiples of 1/64 in (-1, 1))
            const float xf = (float)(X - in.ix);
            const float fx = (float)in.fx64 * 0.015625f;
            float cx[N];
#pragma unroll
            for (int i = 0; i < N; ++i) cx[i] = (xf + (off[i] - fx)) / scale;
            float cy[N];
#pragma unroll
            for (int j = 0; j < N; ++j) cy[j] = ((float)(in.pen_y - Y) - off[j]) / scale;
            int wn[N * N];
#pragma unroll
            for (int k = 0; k < N * N; ++k) wn[k] = 0;
            const Rec *recs = a.recs + in.rec;
            const uint32_t nr = a.rec_count[in.glyph];
            for (uint32_t r = 0; r < nr; ++r) {
                const Rec rc = recs[r];
#pragma unroll
                for (int j = 0; j < N; ++j) {
                    if (cy[j] >= rc.lo && cy[j] <= rc.hi) {                // [lo, hi] contains the accepted heights
                        float xx;
                        int sgn;
                        if (rec_cross<FILL>(rc, cy[j], xx, sgn)) {
#pragma unroll
                            for (int i = 0; i < N; ++i) wn[j * N + i] += !(xx < cx[i]) ? sgn : 0;
                        }
                    }
                }
            }
            uint32_t m = 0u;
#pragma unroll
            for (int k = 0; k < N * N; ++k) m |= (wn[k] != 0 ? 1u : 0u) << k;
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

}  // namespace fr

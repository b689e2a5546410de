// fr_layer_shadow.hip — the stages of fr_layer_shadow (include/fr_raster.h; DESIGN.md sections 4.9 and 5): a square maximum
// or a box sum over the alpha of a layer or of an intermediate plane, written to the next plane or tinted into the
// destination.  One kernel, instantiated per input, operation and output; the host side (fr_layer_shadow_plan.cpp) lists
// the stages and their rectangles.
#include "fr_layer_shadow.hpp"
#include "fr_layer_tint.hpp"

namespace fr {

namespace {

constexpr uint32_t T = SHADOW_TILE, THREADS = 256;

__device__ __forceinline__ int32_t clamp_to(int64_t v, int32_t hi) { return (int32_t)(v < 0 ? 0 : v > hi ? hi : v); }

}  // namespace

// One workgroup of 256 threads makes one 64 x 64 tile of the stage's output; blockIdx.x counts the tiles row by row.
//   1. The tile's input and a halo of `radius` around it go into LDS as bytes, rows of shadow_lds_pitch(radius): wave w takes
//      rows w, w + 4, ..; a pixel outside the input's extent is 0 and not loaded.  The layer is read as words, of which the
//      top byte is kept.
//   2. Rows.  Box: thread (row, half) keeps a running sum along its row and writes the 32 sums of 2 radius + 1 bytes of its
//      half as 16-bit values (at most 65 * 255); a lane's rows are an odd number of banks apart.  Maximum: every thread takes
//      its share of the (64 + 2 radius) x 64 row maxima.
//   3. Columns.  Box: thread (column, quarter) keeps a running sum of the row sums down its 16 rows and divides each by
//      W = (2 radius + 1)^2 with the reciprocal of ShadowRecip (one v_mul_hi_u32 and a shift, exact).  Maximum: as in 2.
//      The 64 x 64 result bytes go where the input bytes were.
//   4. Out.  A plane: 16 bytes per thread, each row a whole number of tiles.  The destination: every thread first makes
//      one entry of the tint of all 256 alphas in LDS; then four pixels per thread and row, one 16-byte store where the
//      four are inside the rectangle and `vec` says that the rectangle's rows sit on the 16-byte grid shifted by `lead`,
//      else pixel by pixel and only inside the rectangle.
// With SHADOW_OP_NONE steps 2 and 3 are left out: the tile is extracted and tinted.
template <int IN_LAYER, int OP, int TINT>
__global__ __launch_bounds__(THREADS) void layer_shadow_kernel(ShadowArgs a)
{
    extern __shared__ uint4 lds_raw[];
    const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
    const uint32_t rho = OP == SHADOW_OP_NONE ? 0u : a.radius;
    const uint32_t LW = T + 2u * rho, IP = shadow_lds_pitch(rho);
    uint8_t *const in = reinterpret_cast<uint8_t *>(lds_raw);
    uint16_t *const H = reinterpret_cast<uint16_t *>(in + LW * IP);
    constexpr uint32_t HP = SHADOW_SUM_PITCH;

    [[maybe_unused]] const uint32_t *lut = nullptr;             // the tint of every alpha: only the instances that tint keep it
    if constexpr (TINT) {
        __shared__ uint32_t lds_lut[256];
        lds_lut[t] = tint_of(t, a.rgba, a.srgb);
        lut = lds_lut;
    }

    const uint32_t tile_x = blockIdx.x % a.tiles_x, tile_y = blockIdx.x / a.tiles_x;
    // ---- 1. the input tile
    {
        const int64_t bx = (int64_t)tile_x * T - a.lead + a.off_x - rho, by = (int64_t)tile_y * T + a.off_y - rho;
        const uint32_t c0 = clamp_to(-bx, LW), c1 = clamp_to((int64_t)a.in_w - bx, LW);
        const uint32_t r0 = clamp_to(-by, LW), r1 = clamp_to((int64_t)a.in_h - by, LW);
        for (uint32_t r = wave; r < LW; r += THREADS / 64) {
            const bool row_in = r >= r0 && r < r1;
            const uint64_t row_at = row_in ? (uint64_t)(by + r) * a.in_pitch : 0u;
            for (uint32_t c = lane; c < LW; c += 64) {
                uint32_t v = 0u;
                if (row_in && c >= c0 && c < c1) {
                    const uint64_t at = row_at + (uint64_t)(bx + c);
                    v = IN_LAYER ? static_cast<const uint32_t *>(a.in)[at] >> 24 : static_cast<const uint8_t *>(a.in)[at];
                }
                in[r * IP + c] = (uint8_t)v;
            }
        }
    }
    __syncthreads();
    const uint8_t *res = in;                                   // the tile's result bytes and their row pitch
    uint32_t RP = IP;
    if constexpr (OP != SHADOW_OP_NONE) {
        // ---- 2. rows
        if constexpr (OP == SHADOW_OP_BOX) {
            const uint32_t half = t >= LW ? 1u : 0u, row = t - half * LW;
            if (row < LW) {
                const uint8_t *p = in + row * IP + 32u * half;
                uint16_t *h = H + row * HP + 32u * half;
                uint32_t acc = 0u;
                for (uint32_t c = 0; c <= 2u * rho; ++c) acc += p[c];
                h[0] = (uint16_t)acc;
#pragma unroll 8
                for (uint32_t x = 1; x < 32u; ++x) {
                    acc += (uint32_t)p[x + 2u * rho] - (uint32_t)p[x - 1u];
                    h[x] = (uint16_t)acc;
                }
            }
        } else {
            for (uint32_t i = t; i < LW * T; i += THREADS) {
                const uint32_t y = i / T, x = i % T;
                const uint8_t *p = in + y * IP + x;
                uint32_t m = 0u;
                for (uint32_t c = 0; c <= 2u * rho; ++c) m = max(m, (uint32_t)p[c]);
                H[y * HP + x] = (uint16_t)m;
            }
        }
        __syncthreads();
        // ---- 3. columns
        uint8_t *outb = in;
        if constexpr (OP == SHADOW_OP_BOX) {
            const uint32_t x = lane, y0 = 16u * wave;
            const uint16_t *p = H + y0 * HP + x;
            uint32_t acc = 0u;
            for (uint32_t j = 0; j <= 2u * rho; ++j) acc += p[j * HP];
            outb[y0 * T + x] = (uint8_t)(__umulhi(acc + a.half_w, a.recip_m) >> a.recip_shift);
#pragma unroll 8
            for (uint32_t y = 1; y < 16u; ++y) {
                acc += (uint32_t)p[(y + 2u * rho) * HP] - (uint32_t)p[(y - 1u) * HP];
                outb[(y0 + y) * T + x] = (uint8_t)(__umulhi(acc + a.half_w, a.recip_m) >> a.recip_shift);
            }
        } else {
            for (uint32_t i = t; i < T * T; i += THREADS) {
                const uint32_t y = i / T, x = i % T;
                const uint16_t *p = H + y * HP + x;
                uint32_t m = 0u;
                for (uint32_t j = 0; j <= 2u * rho; ++j) m = max(m, (uint32_t)p[j * HP]);
                outb[y * T + x] = (uint8_t)m;
            }
        }
        __syncthreads();
        res = outb;
        RP = T;
    }
    // ---- 4. out
    if constexpr (!TINT) {
        const uint32_t row = t >> 2, seg = t & 3u, y = tile_y * T + row;
        if (y < a.out_h)
            *reinterpret_cast<uint4 *>(static_cast<uint8_t *>(a.out) + ((uint64_t)y * a.out_pitch + (uint64_t)tile_x * T + 16u * seg)) =
                *reinterpret_cast<const uint4 *>(res + row * RP + 16u * seg);
    } else {
        const uint32_t g = t & 15u;
        const int64_t X0 = (int64_t)tile_x * T + 4u * g - a.lead;             // the rectangle's column of the group's first pixel
        uint32_t valid = 0u;
#pragma unroll
        for (uint32_t i = 0; i < 4u; ++i) valid |= (X0 + i >= 0 && X0 + i < (int64_t)a.out_w) ? 1u << i : 0u;
        if (!valid) return;
#pragma unroll
        for (uint32_t it = 0; it < 4u; ++it) {
            const uint32_t row = 16u * it + (t >> 4), y = tile_y * T + row;
            if (y >= a.out_h) continue;
            const uint32_t al = *reinterpret_cast<const uint32_t *>(res + row * RP + 4u * g);
            uint32_t *p = static_cast<uint32_t *>(a.out) + ((int64_t)((uint64_t)y * a.out_pitch) + X0);
            store_tinted4(p, al, valid, a.vec, lut);
        }
    }
}

hipError_t launch_layer_shadow(bool in_layer, ShadowOp op, bool tint, ShadowArgs a, hipStream_t stream)
{
    using Kern = void (*)(ShadowArgs);
    static const Kern kern[2][3][2] = {
        {{layer_shadow_kernel<0, SHADOW_OP_BOX, 0>, layer_shadow_kernel<0, SHADOW_OP_BOX, 1>},
         {layer_shadow_kernel<0, SHADOW_OP_MAX, 0>, layer_shadow_kernel<0, SHADOW_OP_MAX, 1>},
         {nullptr, nullptr}},
        {{layer_shadow_kernel<1, SHADOW_OP_BOX, 0>, layer_shadow_kernel<1, SHADOW_OP_BOX, 1>},
         {layer_shadow_kernel<1, SHADOW_OP_MAX, 0>, layer_shadow_kernel<1, SHADOW_OP_MAX, 1>},
         {nullptr, layer_shadow_kernel<1, SHADOW_OP_NONE, 1>}},
    };
    const Kern k = kern[in_layer][op][tint];
    if (!k) return hipErrorInvalidValue;
    const uint64_t tiles_x = ((uint64_t)a.out_w + a.lead + T - 1) / T, tiles_y = ((uint64_t)a.out_h + T - 1) / T;
    if (!tiles_x || !tiles_y) return hipSuccess;
    if (tiles_x * tiles_y > SHADOW_MAX_TILES) return hipErrorInvalidValue;     // (the planner refuses such rectangles)
    a.tiles_x = (uint32_t)tiles_x;
    hipLaunchKernelGGL(k, dim3((uint32_t)(tiles_x * tiles_y)), dim3(THREADS), shadow_lds_bytes(op, op == SHADOW_OP_NONE ? 0u : a.radius), stream, a);
    return hipGetLastError();
}

}  // namespace fr

// fr_layer_shadow.hpp — what the shadow kernel (fr_layer_shadow.hip) reads and how fr_api_layer.hip launches it
#pragma once
#include "fr_layer_shadow_plan.hpp"

#include <hip/hip_runtime.h>

namespace fr {

// One stage: output pixel (x, y), 0 <= x < out_w, 0 <= y < out_h, is made from the input pixels (x + off_x + i, y + off_y + j),
// |i|, |j| <= radius, where an input pixel outside [0, in_w) x [0, in_h) counts as 0 and is not loaded.
struct ShadowArgs {
    const void *in;            // layer input: the window's first pixel (4-byte words, alpha in the top byte); else a plane's first byte
    void *out;                 // a plane's first byte, or the destination rectangle's first pixel
    uint64_t in_pitch, out_pitch;      // elements of their kind
    int64_t off_x, off_y;
    uint32_t in_w, in_h, out_w, out_h;
    uint32_t radius;           // 0 for SHADOW_OP_NONE
    uint32_t recip_m, recip_shift, half_w;     // the box division: (sum + half_w) div W as a multiply (ShadowRecip)
    uint32_t lead;             // tint: the tile columns start this many pixels left of the rectangle, on the 16-byte grid; `vec`
    uint32_t vec;              // says that whole groups of four pixels may go as one 16-byte store
    uint32_t rgba;             // tint: R | G << 8 | B << 16 | A << 24
    uint32_t srgb;             // tint: FR_LAYER_SRGB
    uint32_t tiles_x;          // tile columns: blockIdx.x = tile row * tiles_x + tile column (set by the launch)
};

enum ShadowOp : int { SHADOW_OP_BOX = 0, SHADOW_OP_MAX = 1, SHADOW_OP_NONE = 2 };

// the rows (and columns) of a workgroup's input tile, its row pitch in LDS (bytes: a multiple of 4, an odd number of banks)
// and the dynamic LDS of one workgroup
constexpr uint32_t shadow_lds_rows(uint32_t radius) { return SHADOW_TILE + 2 * radius; }
constexpr uint32_t shadow_lds_pitch(uint32_t radius)
{
    const uint32_t p = (shadow_lds_rows(radius) + 3u) & ~3u;
    return (p >> 2) & 1u ? p : p + 4u;
}
constexpr uint32_t SHADOW_SUM_PITCH = SHADOW_TILE + 2;         // 16-bit row sums: 33 banks a row
constexpr size_t shadow_lds_bytes(ShadowOp op, uint32_t radius)
{
    return (size_t)shadow_lds_rows(radius) * shadow_lds_pitch(radius) + (op == SHADOW_OP_NONE ? 0 : (size_t)shadow_lds_rows(radius) * SHADOW_SUM_PITCH * 2);
}

// layer_shadow_kernel<in_layer, op, tint> over all tiles of a.out_w + a.lead by a.out_h pixels, one launch.  in_layer: the
// input is the layer; tint: the output is the destination (else a plane).
hipError_t launch_layer_shadow(bool in_layer, ShadowOp op, bool tint, ShadowArgs a, hipStream_t stream);

}  // namespace fr

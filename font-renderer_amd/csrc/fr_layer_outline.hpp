// fr_layer_outline.hpp — what the outline kernel (fr_layer_outline.hip) reads and how fr_api_layer.hip launches it
#pragma once
#include "fr_layer_outline_plan.hpp"

#include <hip/hip_runtime.h>

namespace fr {

// Output pixel (x, y) of the rectangle, 0 <= x < out_w, 0 <= y < out_h, shows window coordinate (x + off_x, y + off_y); a
// window pixel outside [0, in_w) x [0, in_h) counts as 0 and is not loaded.
struct OutlineArgs {
    const uint32_t *in;        // the window's first pixel (alpha in the top byte)
    uint32_t *out;             // the destination rectangle's first pixel
    const uint4 *table;        // OutlineTable::packed on the device,
    uint32_t units;            // its units of 16 bytes: at most OUTLINE_MAX_UNITS
    uint64_t in_pitch, out_pitch;      // pixels
    int64_t off_x, off_y;
    uint32_t in_w, in_h, out_w, out_h;
    uint32_t live_x0, live_y0, live_x1, live_y1;       // OutlinePlan::live in the rectangle's coordinates
    uint32_t reach;            // R
    uint32_t levels;           // OutlineTable::levels
    uint32_t lead, vec;        // as ShadowArgs
    uint32_t rgba;             // R | G << 8 | B << 16 | A << 24
    uint32_t srgb;             // FR_LAYER_SRGB
    uint32_t tiles_x;          // blockIdx.x = tile row * tiles_x + tile column
};

// A workgroup's input in LDS: SHADOW_TILE + 2 R rows of outline_lds_words(R) words; tile column x is byte x + R4 of its row,
// R4 = R rounded up to whole words, and one more word lets every window of four bytes be cut from two whole words.  The
// pitch is an odd number of banks.  `levels` running-maximum levels of the same shape follow it.
constexpr uint32_t outline_lds_words(uint32_t reach) { return SHADOW_TILE / 4u + ((reach + 3u) & ~3u) / 2u + 1u; }
constexpr size_t outline_lds_bytes(uint32_t reach, uint32_t levels) { return (size_t)(levels + 1u) * (SHADOW_TILE + 2u * reach) * outline_lds_words(reach) * 4u; }

// the levels of the widest core there is, 2 OUTLINE_MAX_REACH + 1 = 33 bytes
constexpr uint32_t OUTLINE_MAX_LEVELS = 5;

// the largest table: 2 R + 1 rows and their weights at R = OUTLINE_MAX_REACH
constexpr uint32_t OUTLINE_MAX_UNITS =
    (2u * OUTLINE_MAX_REACH + 1u) + ((2u * OUTLINE_MAX_REACH + 1u) * outline_row_words(FR_OUTLINE_MAX_RADIUS) + 3u) / 4u;

// layer_outline_kernel<complement, post> for `kind` over tiles_x * tiles_y tiles, one launch
hipError_t launch_layer_outline(uint32_t kind, uint32_t tiles, const OutlineArgs &a, hipStream_t stream);

}  // namespace fr

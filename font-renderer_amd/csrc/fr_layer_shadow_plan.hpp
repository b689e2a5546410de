// fr_layer_shadow_plan.hpp — the host side of fr_layer_shadow (include/fr_raster.h; DESIGN.md sections 4.9 and 5): the
// argument checks, the stage list with the rectangle every stage has to produce, the reciprocal of the box division and
// the size of the two intermediate planes.  Plain C++, no HIP: device pointers come in as integers.
// host/layer_shadow_selftest.cpp runs all of it on the CPU.
#pragma once
#include "../../include/fr_raster.h"

#include <cstddef>
#include <cstdint>
#include <vector>

namespace fr {

// A stage kernel's workgroup makes one SHADOW_TILE x SHADOW_TILE tile of its stage's output from that tile and a halo of
// the stage's radius around it.  A plane row holds a whole number of tiles.
constexpr uint32_t SHADOW_TILE = 64;
constexpr uint32_t SHADOW_MAX_SPREAD = 8, SHADOW_MAX_RADIUS = 32, SHADOW_MAX_PASSES = 3;
// the two intermediate planes together: FR_E_UNSUPPORTED beyond
constexpr uint64_t SHADOW_MAX_PLANE_BYTES = (uint64_t)1 << 30;
constexpr size_t SHADOW_MAX_ROWS = 0x7fffffffu;
// a destination rectangle may need at most this many tiles (2^34 pixels, fr_layer_over's limit): FR_E_UNSUPPORTED beyond.  The
// tint's tile columns may start up to three pixels left of the rectangle, which counts.
constexpr uint64_t SHADOW_MAX_TILES = (uint64_t)1 << 22;

enum ShadowKind : uint32_t { SHADOW_BOX = 0, SHADOW_SPREAD = 1 };

// half open, in window coordinates (u, v): the window itself is [0, w) x [0, h).  Empty: all four zero.
struct ShadowRect {
    int64_t x0, y0, x1, y1;
    bool empty() const { return x0 >= x1 || y0 >= y1; }
    uint64_t w() const { return (uint64_t)(x1 - x0); }
    uint64_t h() const { return (uint64_t)(y1 - y0); }
};

// n div W for every n <= 255 W + W div 2, W = (2 r + 1)^2, as (n * m) >> (32 + shift) with m = ceil(2^(32 + shift) / W) and
// shift = floor(log2 W): m is below 2^32, and with e = m W - 2^(32 + shift) < W < 2^(shift + 1) and n < 2^21 the error term
// n e is below 2^(shift + 22) <= 2^(32 + shift), which is the condition for the floor to be exact.
// tests/test_layer_shadow_ref.py checks every numerator of every radius.
struct ShadowRecip {
    uint32_t m, shift;
};
ShadowRecip shadow_recip(uint32_t radius);

struct ShadowStage {
    ShadowKind kind;
    uint32_t radius;           // s of the spread, r of a box pass: at least 1
    ShadowRect out;            // what the stage must produce: the destination rectangle moved by (-dx, -dy), grown by the radii
                               // still to come, cut to where the stage's output can be non-zero (the window grown by the radii
                               // up to and including this one).  The last stage writes the whole destination rectangle, zeros
                               // outside `out`; the others write `out` into a plane.
    uint64_t pitch;            // of that plane, bytes: out.w() rounded up to whole tiles (0 for the last stage)
    ShadowRecip recip;         // SHADOW_BOX
};

struct ShadowIn {
    uintptr_t src, dst;        // the two device pointers
    size_t src_stride, src_rows, dst_stride, dst_rows;
    const fr_layer_shadow_params *shadow;
    uint32_t flags;
};

struct ShadowPlan {
    bool nothing = true;               // dst_w or dst_h is 0: no launch
    bool zeros = false;                // the rectangle is out of the shadow's reach (or the window has no area): one launch that
                                       // writes zeros, no stage
    ShadowRect want{0, 0, 0, 0};       // the destination rectangle in window coordinates
    std::vector<ShadowStage> stages;   // in order; empty with !zeros: one launch that extracts and tints
    uint64_t plane_bytes[2] = {0, 0};  // stage k (from 0) writes plane k & 1
};

// The checks of fr_layer_shadow in the order the header lists them, then the stages.  FR_OK, or the code with its message
// left through fr::set_error; `out` is only meaningful after FR_OK.
int shadow_plan(const ShadowIn &in, ShadowPlan &out);

}  // namespace fr

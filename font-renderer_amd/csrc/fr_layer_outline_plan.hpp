// fr_layer_outline_plan.hpp — the host side of fr_layer_outline (include/fr_raster.h; DESIGN.md sections 4.13 and 5): the
// argument checks, the destination rectangle in window coordinates and its cut to where the outline can be non-zero, the
// tile counts and the table of disc weights.  Plain C++, no HIP: device pointers come in as integers.
// host/layer_outline_selftest.cpp runs all of it on the CPU.
#pragma once
#include "fr_layer_shadow_plan.hpp"            // ShadowRect, and the tile and its limits, which the outline shares

namespace fr {

constexpr uint32_t OUTLINE_MAX_REACH = (FR_OUTLINE_MAX_RADIUS + 15u) / 16u;

// the reach R = ceil(rho / 16) in pixels; the kernel's halo in columns is R rounded up to whole words of four bytes
constexpr uint32_t outline_reach(uint32_t rho) { return (rho + 15u) / 16u; }
constexpr uint32_t outline_reach4(uint32_t rho) { return (outline_reach(rho) + 3u) & ~3u; }
// a kernel row's weights as words of four: tap t = i + outline_reach4 of 0 .. 2 outline_reach4 + 3 is byte t % 4 of word t / 4
constexpr uint32_t outline_row_words(uint32_t rho) { return outline_reach4(rho) / 2u + 1u; }

// K(i, j) of the header: 0 .. 255
uint32_t outline_weight(uint32_t rho, int32_t i, int32_t j);

// One kernel row j, 16 bytes.  K(i, j) is 255 for |i| <= core (core = -1: nowhere), strictly between 0 and 255 for
// core < |i| <= core + rim, and 0 beyond; level = floor(log2(2 core + 1)) is the running-maximum level whose windows of
// 2^level bytes, two of them, cover the core (0 without a core).
struct OutlineRow {
    int32_t core;
    uint32_t rim, level, unused;
};

struct OutlineTable {
    uint32_t reach = 0, reach4 = 0, row_words = 0;
    uint32_t levels = 0;               // the largest level of a row: the running-maximum levels the kernel builds
    std::vector<uint8_t> k;            // (2 reach + 1)^2: K(i, j) at [(j + reach) * (2 reach + 1) + i + reach]
    std::vector<OutlineRow> rows;      // 2 reach + 1
    // what the kernel reads, in units of 16 bytes: the rows, then row_words words of weights per row (zero beyond |i| = reach)
    // from a 16-byte boundary, the last unit filled up with zeros
    std::vector<uint32_t> packed;
    size_t units() const { return packed.size() / 4; }
};
void outline_table(uint32_t rho, OutlineTable &out);

struct OutlineIn {
    uintptr_t src, dst;        // the two device pointers
    size_t src_stride, src_rows, dst_stride, dst_rows;
    const fr_layer_outline_params *outline;
    uint32_t flags;
};

struct OutlinePlan {
    bool nothing = true;               // dst_w or dst_h is 0: no launch
    bool zeros = false;                // every pixel of the rectangle is (0, 0, 0, 0): out of reach, a window without area, or
                                       // RING or INNER at radius 0; one launch that writes zeros, no table
    ShadowRect want{0, 0, 0, 0};       // the destination rectangle in window coordinates
    ShadowRect live{0, 0, 0, 0};       // `want` cut to where alpha can be non-zero: the window grown by the reach (GROW, RING) or
                                       // the window (INNER, SHRINK).  A tile outside it writes zeros without loading.
    uint32_t vec = 0, lead = 0;        // the stores: rows on the 16-byte grid shifted by `lead` pixels (fr_layer_shadow.hpp)
    uint64_t tiles_x = 0, tiles_y = 0; // tiles of (dst_w + lead) x dst_h
    OutlineTable table;                // !nothing && !zeros
};

// The checks of fr_layer_outline in the order the header lists them, then the plan.  FR_OK, or the code with its message
// left through fr::set_error; `out` is only meaningful after FR_OK.
int outline_plan(const OutlineIn &in, OutlinePlan &out);

}  // namespace fr

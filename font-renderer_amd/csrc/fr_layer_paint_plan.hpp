// fr_layer_paint_plan.hpp — the host side of fr_layer_paint (include/fr_raster.h; DESIGN.md sections 4.11 and 5): the
// argument checks, the clipping of the rectangle, the gradient's coefficients and its colour table.  Plain C++, no HIP:
// device pointers come in as integers.  host/layer_paint_selftest.cpp runs all of it on the CPU.
#pragma once
#include "fr_layer_plan.hpp"

namespace fr {

constexpr uint32_t PAINT_TABLE = 1024;                 // entries of the colour table G; a pixel reads G[u >> 6]
constexpr int64_t PAINT_MAX_COORD = (int64_t)1 << 26;  // |geometry value| beyond: FR_E_UNSUPPORTED
constexpr int64_t PAINT_MIN_L2 = 4096, PAINT_MIN_R = 64;   // a gradient shorter than one pixel: FR_E_UNSUPPORTED
constexpr int64_t PAINT_MAX_DD = (int64_t)1 << 27;     // radial: |ddx|, |ddy| stay below, so (ddx^2 + ddy^2) 256 < 2^63

struct PaintIn {
    uintptr_t src, dst;        // the two device pointers; src may be 0 (full coverage)
    size_t src_stride, src_rows, dst_stride, dst_rows;
    const fr_layer_paint_params *paint;
    uint32_t flags;
};

// What layer_paint_kernel needs.  The clipped rectangle is [x0, x1) x [y0, y1) of the destination and shows the layer from
// (sx, sy); its tiles are tiles_x x tiles_y of LAYER_TILE_W x LAYER_TILE_H, the first at (tx0, y0) with tx0 = x0 rounded
// down to LAYER_LANE_PX, so that a lane's group of four starts on a multiple of four columns; sx0: the layer column of tx0
// (below zero by up to three when the window starts at column 0).
struct PaintPlan {
    bool nothing = true;       // w or h is 0, or the rectangle is clipped away: nothing is launched, the rest is unset
    uint32_t x0 = 0, y0 = 0, x1 = 0, y1 = 0, sx = 0, sy = 0;
    uint32_t tx0 = 0, tiles_x = 0, tiles_y = 0;
    int32_t sx0 = 0;
    bool dst_vec = false, src_vec = false;     // a lane's group moves as one 16-byte access (LAYER_DST_VEC's, LAYER_SRC_VEC's condition)
    int64_t c[3] = {0, 0, 0};                  // linear: T0, TX, TY; radial: x0, y0, R
    uint32_t table[PAINT_TABLE];               // G: R | G << 8 | B << 16 | A << 24, straight
};

// rdiv(n, d) = floor((2 n + d) / (2 d)) for d > 0 and n of either sign (floor, not truncation: half-way cases go up)
int64_t paint_rdiv(__int128 n, int64_t d);

// The checks of fr_layer_paint in the order the header lists them (after the NULL context), then clipping, the
// coefficients and the table.  FR_OK, or the code with its message left through fr::set_error; `out` is only meaningful
// after FR_OK.
int layer_paint_plan(const PaintIn &in, PaintPlan &out);

}  // namespace fr

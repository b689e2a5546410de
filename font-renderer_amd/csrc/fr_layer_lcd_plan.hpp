// fr_layer_lcd_plan.hpp — the host side of fr_layer_lcd (include/fr_raster.h; DESIGN.md sections 4.12 and 5): the argument
// checks, the clipping of the blits, their overlap check and the tile table the kernel walks, each tile with its blit's
// colour and window.  The clipping, the sweep and the tiling are fr_layer_plan.hpp's.  Plain C++, no HIP: device pointers
// come in as integers.  host/layer_lcd_selftest.cpp runs all of it on the CPU.
#pragma once
#include "fr_layer_plan.hpp"

namespace fr {

// A tile of one clipped blit, in destination pixels, as LayerTile: x is a multiple of LAYER_LANE_PX at or below the
// rectangle's left edge, and lane l's group starts at column x + 4 l.  sq: the plane element of sub-pixel 0 of column x in
// the plane row sy of y (below zero by up to nine when x < x0 and the window starts at element 0).  [q0, q1): the window's
// elements in every one of its rows; an element outside counts as 0 and is not read.
struct LcdTile {
    uint32_t x, y;
    uint32_t x0, x1, y1;
    uint32_t sy;
    int32_t sq;
    uint32_t q0, q1;
    uint32_t rgba;             // the blit's colour: byte b of the pixel in bits 8 b .. 8 b + 7, A on top
    uint32_t vec;              // LAYER_DST_VEC | LAYER_SRC_VEC (the plane's dwords)
    uint32_t unused;
};
static_assert(sizeof(LcdTile) == 48, "LcdTile is three dwordx4");

struct LcdIn {
    uintptr_t cov, dst;        // the two device pointers
    size_t cov_stride, cov_rows, dst_stride, dst_rows;
    const fr_lcd_blit *blits;
    uint32_t n_blits;
    const uint16_t *weights;   // FR_LCD_TAPS values, or nullptr: the default filter
    uint32_t flags;
};

struct LcdTables {
    std::vector<LayerClip> clips;      // one per blit, in the caller's order; sx: the window's pixel column of x0
    std::vector<LcdTile> tiles;        // blit by blit, rows of tiles top to bottom, left to right
    uint32_t w[FR_LCD_TAPS] = {0, 0, 0, 0, 0};
};

constexpr uint16_t LCD_DEFAULT_WEIGHTS[FR_LCD_TAPS] = {8, 77, 86, 77, 8};

// The checks of fr_layer_lcd in the order the header lists them (after the NULL context), then clipping, the overlap
// check and the tiles.  FR_OK, or the code with its message left through fr::set_error; `out` is only meaningful after
// FR_OK.
int layer_lcd_tables(const LcdIn &in, LcdTables &out);

}  // namespace fr

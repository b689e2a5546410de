// fr_layer_rects_plan.hpp — the host side of fr_layer_rects (include/fr_raster.h; DESIGN.md sections 4.10 and 5): the
// argument checks, the clipping of the rectangles and the three tables the kernel walks.  Plain C++, no HIP: the device
// pointer comes in as an integer.  host/layer_rects_selftest.cpp runs all of it on the CPU.
#pragma once
#include "fr_layer_plan.hpp"

namespace fr {

// a call may list at most this many (tile, rectangle) pairs: FR_E_UNSUPPORTED beyond (and LAYER_MAX_TILES tiles)
constexpr uint64_t RECTS_MAX_PAIRS = (uint64_t)1 << 24;
// edges of int32 in 1/64 pixel end here: no column or row at or beyond 2^25 is ever drawn into
constexpr int64_t RECTS_MAX_EDGE = 0x7fffffff;

// A rectangle that draws, clipped to the image: edges in 1/64 pixel, x0 < x1 <= min(64 stride, 2^31 - 1), y likewise.
struct RectRec {
    uint32_t x0, y0, x1, y1;
    uint32_t rgba;             // R | G << 8 | B << 16 | A << 24, straight; A != 0
    uint32_t index;            // the caller's index of it
    uint32_t pad[2];
};
static_assert(sizeof(RectRec) == 32, "RectRec is two dwordx4");

// A tile of the image's own grid (x a multiple of LAYER_TILE_W, y of LAYER_TILE_H) that some record meets, and its records:
// list[first .. first + count), ascending, which is the caller's order.
struct RectTile {
    uint32_t x, y, first, count;
};
static_assert(sizeof(RectTile) == 16, "RectTile is one dwordx4");

struct RectsIn {
    uintptr_t dst;             // the device pointer
    size_t dst_stride, dst_rows;
    const fr_layer_rect *rects;
    uint32_t n_rects;
    uint32_t flags;
};

struct RectsTables {
    std::vector<RectRec> recs;         // the rectangles that draw, in the caller's order
    std::vector<RectTile> tiles;       // top to bottom, left to right
    std::vector<uint32_t> list;        // indices into recs, tile by tile
    bool dst_vec = false;              // LAYER_DST_VEC's condition: 16-byte aligned rows, so a lane's group moves as one access
};

// The checks of fr_layer_rects in the order the header lists them (after the NULL context), then clipping and binning.
// FR_OK, or the code with its message left through fr::set_error; `out` is only meaningful after FR_OK.
int layer_rects_tables(const RectsIn &in, RectsTables &out);

}  // namespace fr

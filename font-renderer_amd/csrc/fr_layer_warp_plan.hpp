// fr_layer_warp_plan.hpp — the host side of fr_layer_warp (include/fr_raster.h; DESIGN.md sections 4.15 and 5): the argument
// checks in the header's order, the clipping of the rectangles, their overlap check, the culling of the tiles that no tap
// can reach and the tile table the kernel walks.  The clipping, the overlap sweep and the image check are
// fr_layer_plan.hpp's.  Plain C++, no HIP: device pointers come in as integers.  host/layer_warp_selftest.cpp runs all of
// it on the CPU.
#pragma once
#include "fr_layer_plan.hpp"

namespace fr {

// One workgroup of LAYER_WAVES waves takes one tile of WARP_TILE x WARP_TILE pixels: a lane owns LAYER_LANE_PX consecutive
// pixels of a row, a wave eight such groups by eight rows, so that the taps of a wave stay close together under any turn.
constexpr uint32_t WARP_TILE = 32;
constexpr int64_t WARP_ONE = 65536, WARP_HALF = 32768;
constexpr int64_t WARP_MAX_ORIGIN = (int64_t)1 << 47;          // |u0|, |v0|
constexpr uint32_t WARP_MAX_RECT = 1u << 26;                   // dst_w, dst_h

// A tile of one clipped rectangle, in destination pixels.  x is a multiple of LAYER_LANE_PX at or below the rectangle's left
// edge and the pixels of the tile are [max(x, x0), min(x + WARP_TILE, x1)) by [y, min(y + WARP_TILE, y1)), as LayerTile's.
// (U, V): the window position that the centre of pixel (x, y) samples, extrapolated where x < x0.  (wx, wy, ww, wh): the
// blit's window in the layer.  [i0, i1] x [j0, j1]: the window pixels that the taps of the tile's pixels can touch, a box
// inside the window that is never empty; the kernel loads from no other pixel.
struct WarpTile {
    uint32_t x, y, x0, x1;
    uint32_t y1, ov, wx, wy;   // ov: opacity | LAYER_DST_VEC
    int64_t U, V;
    int32_t ux, uy, vx, vy;
    uint32_t ww, wh, i0, j0;
    uint32_t i1, j1, pad[2];
};
static_assert(sizeof(WarpTile) == 96, "WarpTile is six dwordx4");

struct WarpIn {
    uintptr_t src, dst;        // the two device pointers
    size_t src_stride, src_rows, dst_stride, dst_rows;
    const fr_layer_warp_blit *blits;
    uint32_t n_blits;
    uint32_t flags;
};

struct WarpTables {
    std::vector<LayerClip> clips;      // one per blit, in the caller's order; (sx, sy) is the rectangle pixel (X, Y) of (x0, y0)
    std::vector<WarpTile> tiles;       // blit by blit, rows of tiles top to bottom, left to right; only those a tap can reach
    bool opacity = false;              // some blit that has tiles has an opacity below 255: the OPACITY = 1 instance
    uint64_t pixels = 0;               // sum of the clipped rectangles' areas
    uint64_t walked = 0;               // tiles of the clipped rectangles before the culling (what the 2^22 limit counts)
};

// The smallest and largest of u + X * ux + Y * uy over the corners of [X0, X1] x [Y0, Y1] (inclusive): the extremes of an
// affine function over the box.
inline void warp_extremes(int64_t u, int32_t ux, int32_t uy, int64_t X0, int64_t X1, int64_t Y0, int64_t Y1, int64_t &lo, int64_t &hi)
{
    const int64_t a = u + X0 * ux + Y0 * uy, b = u + X1 * ux + Y0 * uy, c = u + X0 * ux + Y1 * uy, d = u + X1 * ux + Y1 * uy;
    lo = std::min(std::min(a, b), std::min(c, d));
    hi = std::max(std::max(a, b), std::max(c, d));
}

// The checks of fr_layer_warp in the order the header lists them, then clipping, the overlap check, the culling and the
// tiles.  FR_OK, or the code with its message left through fr::set_error; `out` is only meaningful after FR_OK.
int layer_warp_tables(const WarpIn &in, WarpTables &out);

}  // namespace fr

// fr_layer_plan.hpp — the host side of fr_layer_over and fr_layer_unpremultiply (include/fr_raster.h; DESIGN.md sections
// 4.8 and 5): the argument checks, the clipping of the blits, their overlap check and the tile table the kernel walks.
// Plain C++, no HIP: device pointers come in as integers.  host/layer_selftest.cpp runs all of it on the CPU.
#pragma once
#include "../../include/fr_raster.h"

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace fr {

// One workgroup of LAYER_WAVES waves takes one tile: a lane owns LAYER_LANE_PX consecutive pixels of a row (16 bytes), a
// wave a row of 64 such groups, and walks LAYER_TILE_H / LAYER_WAVES rows.
constexpr uint32_t LAYER_LANE_PX = 4, LAYER_TILE_W = 64 * LAYER_LANE_PX, LAYER_TILE_H = 16, LAYER_WAVES = 4;
// a call may list at most this many tiles (2^34 pixels): FR_E_UNSUPPORTED beyond
constexpr uint64_t LAYER_MAX_TILES = (uint64_t)1 << 22;
// rows of either image beyond this: FR_E_UNSUPPORTED (a tile keeps its rows in 32 bits)
constexpr size_t LAYER_MAX_ROWS = 0x7fffffffu;

// LayerTile::ov above the opacity: the lane groups that lie wholly inside [x0, x1) move as one 16-byte access
constexpr uint32_t LAYER_DST_VEC = 0x100u, LAYER_SRC_VEC = 0x200u;

// A tile of one clipped blit, in destination pixels.  x is a multiple of LAYER_LANE_PX at or below the rectangle's left
// edge, so that lane l's group starts at column x + 4 l; the pixels of the tile are [max(x, x0), min(x + LAYER_TILE_W, x1))
// by [y, min(y + LAYER_TILE_H, y1)).  (sx, sy): the layer pixel that lands on (x, y); sx is below zero by up to three when
// x < x0 and the blit reads the layer from column 0 (those pixels are outside the tile).
struct LayerTile {
    uint32_t x, y;
    uint32_t x0, x1, y1;
    int32_t sx;
    uint32_t sy;
    uint32_t ov;               // opacity | LAYER_DST_VEC | LAYER_SRC_VEC
};
static_assert(sizeof(LayerTile) == 32, "LayerTile is two dwordx4");

struct LayerIn {
    uintptr_t src, dst;        // the two device pointers
    size_t src_stride, src_rows, dst_stride, dst_rows;
    const fr_layer_blit *blits;
    uint32_t n_blits;
    uint32_t flags;
};

// a blit clipped to the destination: [x0, x1) x [y0, y1) there (empty: x0 == x1 == 0), from (sx, sy) of the layer
struct LayerClip {
    uint32_t x0, y0, x1, y1;
    uint32_t sx, sy;
};

// The w x h rectangle at (dst_x, dst_y) clipped to [0, dst_stride) x [0, dst_rows), showing its source from (src_x, src_y);
// empty when w or h is 0 or nothing of it is visible.  (fr_layer_lcd passes src_x = 0: sx is then the window's pixel column.)
inline LayerClip layer_clip(uint32_t src_x, uint32_t src_y, uint32_t w, uint32_t h, int32_t dst_x, int32_t dst_y, size_t dst_stride, size_t dst_rows)
{
    if (!w || !h) return LayerClip{0, 0, 0, 0, 0, 0};
    const int64_t x0 = std::max<int64_t>(dst_x, 0), y0 = std::max<int64_t>(dst_y, 0);
    const int64_t x1 = std::min<int64_t>((int64_t)dst_x + w, (int64_t)dst_stride);
    const int64_t y1 = std::min<int64_t>((int64_t)dst_y + h, (int64_t)dst_rows);
    if (x0 >= x1 || y0 >= y1) return LayerClip{0, 0, 0, 0, 0, 0};
    return LayerClip{(uint32_t)x0, (uint32_t)y0, (uint32_t)x1, (uint32_t)y1, (uint32_t)(src_x + (x0 - dst_x)), (uint32_t)(src_y + (y0 - dst_y))};
}

// the clipped rectangles own their pixels: whether two of them overlap, and which (a sweep down the rows, as for text runs)
inline bool layer_clips_overlap(const std::vector<LayerClip> &clips, uint32_t &first, uint32_t &second)
{
    std::vector<uint32_t> ord;
    for (uint32_t b = 0; b < clips.size(); ++b)
        if (clips[b].x0 < clips[b].x1) ord.push_back(b);
    std::sort(ord.begin(), ord.end(), [&](uint32_t p, uint32_t q) { return clips[p].y0 < clips[q].y0; });
    for (size_t i = 0; i < ord.size(); ++i) {
        const LayerClip &A = clips[ord[i]];
        for (size_t j = i + 1; j < ord.size() && clips[ord[j]].y0 < A.y1; ++j) {
            const LayerClip &B = clips[ord[j]];
            if (B.x0 < A.x1 && A.x0 < B.x1) {
                first = ord[i], second = ord[j];
                return true;
            }
        }
    }
    return false;
}

// the tiles of a clipped rectangle that is not empty: their number, and f(x, y) for each, rows of tiles top to bottom, left
// to right, the first at (x0 rounded down to LAYER_LANE_PX, y0)
inline uint64_t layer_clip_tiles(const LayerClip &c)
{
    const uint32_t tx0 = c.x0 & ~(LAYER_LANE_PX - 1);
    return (uint64_t)((c.x1 - tx0 + LAYER_TILE_W - 1) / LAYER_TILE_W) * ((c.y1 - c.y0 + LAYER_TILE_H - 1) / LAYER_TILE_H);
}
template <class F>
inline void layer_each_tile(const LayerClip &c, F f)
{
    for (uint32_t y = c.y0; y < c.y1; y += LAYER_TILE_H)
        for (uint32_t x = c.x0 & ~(LAYER_LANE_PX - 1); x < c.x1; x += LAYER_TILE_W) f(x, y);
}

struct LayerTables {
    std::vector<LayerClip> clips;      // one per blit, in the caller's order
    std::vector<LayerTile> tiles;      // blit by blit, rows of tiles top to bottom, left to right; none for opacity 0
    bool opacity = false;              // some blit that has tiles has an opacity below 255: the OPACITY = 1 instance
    uint64_t pixels = 0;               // sum of the clipped rectangles' areas
};

// The checks of fr_layer_over in the order the header lists them, then clipping, the overlap check (the sweep down the rows
// that text runs use) and the tiles.  FR_OK, or the code with its message left through fr::set_error; `out` is only
// meaningful after FR_OK.
int layer_tables(const LayerIn &in, LayerTables &out);

int set_error(int code, const char *fmt, ...);         // the context unit (the self-tests have their own)

// an image of the layer calls: a non-NULL, 4-byte aligned pointer and a row pitch within fr_plan_render's limit
inline int layer_image_check(const char *what, uintptr_t p, size_t stride)
{
    if (!p) return set_error(FR_E_INVALID, "%s is NULL", what);
    if (p & 3u) return set_error(FR_E_INVALID, "%s %p is not 4-byte aligned", what, (void *)p);
    if (stride > ((size_t)1 << 26)) return set_error(FR_E_INVALID, "%s: row pitch of %zu elements: at most 2^26", what, stride);
    return FR_OK;
}

// the checks of fr_layer_unpremultiply
int layer_window_check(uintptr_t rgba, size_t stride_px, uint32_t w, uint32_t h);

}  // namespace fr

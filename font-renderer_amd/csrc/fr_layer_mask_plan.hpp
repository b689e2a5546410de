// fr_layer_mask_plan.hpp — the host side of fr_layer_mask (include/fr_raster.h; DESIGN.md sections 4.14 and 5): the argument
// checks in the header's order, the clipping of the blits, their overlap check and the tile table the kernel walks.  The
// clipping, the overlap sweep, the tile walk and the image check are fr_layer_plan.hpp's.  Plain C++, no HIP: device
// pointers come in as integers.  host/layer_mask_selftest.cpp runs all of it on the CPU.
#pragma once
#include "fr_layer_plan.hpp"

namespace fr {

// MaskTile::ov beside LAYER_DST_VEC and LAYER_SRC_VEC: the lane groups that lie wholly inside [x0, x1) read their four mask
// elements as one access, 16 bytes of a layer mask or 4 bytes of a plane
constexpr uint32_t LAYER_MASK_VEC = 0x400u;

// LayerTile's fields, then the mask's.  (mx, my): the mask element that lies over (x, y); mx is below zero by up to three
// where sx is.  With FR_MASK_ERASE there is no layer: sx and sy then hold the offset into the blit's rectangle and are not
// used.
struct MaskTile {
    uint32_t x, y;
    uint32_t x0, x1, y1;
    int32_t sx;
    uint32_t sy;
    uint32_t ov;               // opacity | LAYER_DST_VEC | LAYER_SRC_VEC | LAYER_MASK_VEC
    int32_t mx;
    uint32_t my;
    uint32_t invert;           // 0 or 1
    uint32_t pad;
};
static_assert(sizeof(MaskTile) == 48, "MaskTile is three dwordx4");

struct MaskIn {
    uintptr_t src, mask, dst;  // the three device pointers; src is 0 with FR_MASK_ERASE
    size_t src_stride, src_rows, mask_stride, mask_rows, dst_stride, dst_rows;
    const fr_layer_mask_blit *blits;
    uint32_t n_blits;
    uint32_t flags;
};

struct MaskOrigin {            // the mask element over a clipped rectangle's top-left pixel
    uint32_t mx, my;
};

struct MaskTables {
    std::vector<LayerClip> clips;      // one per blit, in the caller's order (FR_MASK_ERASE: clipped as from src (0, 0))
    std::vector<MaskOrigin> origins;   // one per blit; (0, 0) for an empty clip
    std::vector<MaskTile> tiles;       // blit by blit, rows of tiles top to bottom, left to right; none for opacity 0
    uint64_t pixels = 0;               // sum of the clipped rectangles' areas
};

// The checks of fr_layer_mask in the order the header lists them, then clipping, the overlap check and the tiles.  FR_OK, or
// the code with its message left through fr::set_error; `out` is only meaningful after FR_OK.
int layer_mask_tables(const MaskIn &in, MaskTables &out);

}  // namespace fr

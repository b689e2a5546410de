// fr_layer_paint.hpp — what layer_paint_kernel (fr_layer_paint.hip) reads and how fr_api_layer.hip launches it
#pragma once
#include "fr_layer_paint_plan.hpp"

#include <hip/hip_runtime.h>

namespace fr {

struct PaintArgs {             // PaintPlan's fields, the colour table in device memory, and the two images
    const uint32_t *table;     // G[PAINT_TABLE], 16-byte aligned
    const uint32_t *src;       // the layer, or nullptr: full coverage
    uint32_t *dst;
    uint64_t src_stride, dst_stride;   // pixels
    uint32_t x0, x1, y0, y1;   // the clipped rectangle
    uint32_t tx0, tiles_x;
    int32_t sx0;               // the layer column of tx0
    uint32_t sy;               // the layer row of y0
    uint32_t vec;              // LAYER_DST_VEC | LAYER_SRC_VEC
    uint32_t spread;
    int64_t c[3];              // linear: T0, TX, TY; radial: x0, y0, R
};

// layer_paint_kernel<srgb, radial, src != nullptr> over n_tiles = tiles_x * tiles_y tiles, one workgroup each
hipError_t launch_layer_paint(bool srgb, bool radial, uint32_t n_tiles, const PaintArgs &a, hipStream_t stream);

}  // namespace fr

// fr_layer_rects.hpp — what layer_rects_kernel (fr_layer_rects.hip) reads and how fr_api_layer.hip launches it
#pragma once
#include "fr_layer_rects_plan.hpp"

#include <hip/hip_runtime.h>

namespace fr {

struct RectsArgs {             // the three tables of fr_layer_rects_plan.hpp in device memory, and the image
    const RectTile *tiles;
    const uint32_t *list;
    const RectRec *recs;
    uint32_t *dst;
    uint64_t dst_stride;       // pixels
    uint32_t dst_vec;          // RectsTables::dst_vec
};

// layer_rects_kernel<srgb> over n_tiles tiles, one workgroup each
hipError_t launch_layer_rects(bool srgb, uint32_t n_tiles, const RectsArgs &a, hipStream_t stream);

}  // namespace fr

// fr_layer_warp.hpp — what layer_warp_kernel (fr_layer_warp.hip) reads and how fr_api_layer.hip launches it
#pragma once
#include "fr_layer_warp_plan.hpp"

#include <hip/hip_runtime.h>

namespace fr {

struct WarpArgs {
    const WarpTile *tiles;
    const uint32_t *src;       // the layer; never written
    uint32_t *dst;
    uint64_t src_stride, dst_stride;   // pixels
};

// layer_warp_kernel<srgb, opacity> over n_tiles tiles, one workgroup each
hipError_t launch_layer_warp(bool srgb, bool opacity, uint32_t n_tiles, const WarpArgs &a, hipStream_t stream);

}  // namespace fr

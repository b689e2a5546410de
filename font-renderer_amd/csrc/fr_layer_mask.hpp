// fr_layer_mask.hpp — what layer_mask_kernel (fr_layer_mask.hip) reads and how fr_api_layer.hip launches it
#pragma once
#include "fr_layer_mask_plan.hpp"

#include <hip/hip_runtime.h>

namespace fr {

struct MaskArgs {
    const MaskTile *tiles;
    const uint32_t *src;       // the layer (nullptr when erasing); never written
    const void *mask;          // 4-byte pixels whose alpha is the mask value, or a plane of bytes; never written
    uint32_t *dst;
    uint64_t src_stride, mask_stride, dst_stride;      // elements: pixels, or the plane's bytes
};

// layer_mask_kernel<srgb, plane, erase> over n_tiles tiles, one workgroup each
hipError_t launch_layer_mask(bool srgb, bool plane, bool erase, uint32_t n_tiles, const MaskArgs &a, hipStream_t stream);

}  // namespace fr

// fr_layer.hpp — what the layer kernels (fr_layer.hip) read and how fr_api_layer.hip launches them
#pragma once
#include "fr_layer_plan.hpp"

#include <hip/hip_runtime.h>

namespace fr {

struct LayerArgs {             // what layer_over_kernel reads and writes
    const LayerTile *tiles;
    const uint32_t *src;       // the layer: premultiplied pixels, alpha in the top byte of the word; never written
    uint32_t *dst;
    uint64_t src_stride, dst_stride;   // pixels
};

// n units of 16 bytes from `staged` (pinned host memory the device can read) into `table` (device memory), by a kernel
hipError_t launch_layer_table(const uint4 *staged, uint4 *table, uint32_t n, hipStream_t stream);
// layer_over_kernel<srgb, opacity> over n_tiles tiles, one workgroup each
hipError_t launch_layer_over(bool srgb, bool opacity, uint32_t n_tiles, const LayerArgs &a, hipStream_t stream);
// layer_unpremultiply_kernel<srgb> over the w x h window at rgba (w, h > 0)
hipError_t launch_layer_unpremultiply(bool srgb, uint32_t *rgba, uint64_t stride, uint32_t w, uint32_t h, hipStream_t stream);

}  // namespace fr

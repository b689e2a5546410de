// fr_layer_blend.hpp — how fr_api_layer.hip launches the blend kernels (fr_layer_blend.hip).  The arguments are
// layer_over_kernel's (fr_layer.hpp) and the tiles fr_layer_plan.cpp's.
#pragma once
#include "fr_layer.hpp"
#include "fr_layer_blend_math.hpp"

namespace fr {

// layer_blend_kernel<srgb, mode, opacity> over n_tiles tiles, one workgroup each; mode < FR_BLEND_MODES
hipError_t launch_layer_blend(bool srgb, uint32_t mode, bool opacity, uint32_t n_tiles, const LayerArgs &a, hipStream_t stream);

}  // namespace fr

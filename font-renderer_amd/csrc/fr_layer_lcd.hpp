// fr_layer_lcd.hpp — what layer_lcd_kernel (fr_layer_lcd.hip) reads and how fr_api_layer.hip launches it
#pragma once
#include "fr_layer_lcd_plan.hpp"

#include <hip/hip_runtime.h>

namespace fr {

struct LcdArgs {
    const LcdTile *tiles;
    const uint8_t *cov;        // the plane: one byte per element; never written
    uint32_t *dst;
    uint64_t cov_stride, dst_stride;   // bytes; pixels
    uint32_t w[FR_LCD_TAPS];   // the filter
    uint32_t bgr;              // memory byte b takes sub-pixel 2 - b
};

// layer_lcd_kernel<srgb> over n_tiles tiles, one workgroup each
hipError_t launch_layer_lcd(bool srgb, uint32_t n_tiles, const LcdArgs &a, hipStream_t stream);

}  // namespace fr

// fr_text_tables.hpp — the plain tables of a text plan: fr_text_plan.cpp builds them on the host (no HIP), fr_api_plan.hip
// uploads them, the text kernels of fr_text.hip and fr_text_affine.hip read them (fr_text.hpp).  Needs only <cstdint>.
#pragma once
#include <cstdint>

namespace fr {

struct TextInst {      // one placement, resolved on the host (fr_text_plan.cpp)
    int32_t ix;        // floor(pen_x64 / 64)
    int32_t pen_y;     // baseline row
    int32_t x0, x1;    // the cell's columns [x0, x1), clipped to the run (image coordinates)
    int32_t y0, y1;    // its rows [y0, y1), clipped likewise
    uint32_t glyph;    // glyph index (record count: rec_count[glyph])
    uint32_t rec;      // first record of the glyph: 2 * glyph_seg_start[glyph]
    uint32_t fx64;     // pen_x64 mod 64
    uint32_t rgba;     // an RGBA text plan's placement colour, R in the low byte (the bytes R G B A in memory); else 0
    uint32_t pad[2];   // an sRGB text plan's linear colour: D[R] | D[G] << 16, D[B] (fr_srgb.hpp); else 0
};
struct TextInstEx {    // one fr_glyph_place_ex, resolved on the host: TextInst and the placement's own sample map
    int32_t ix;        // floor(pen_x64 / 64)
    int32_t iy;        // floor(pen_y64 / 64)
    int32_t x0, x1;    // the (sheared) cell's columns [x0, x1), clipped to the run
    int32_t y0, y1;    // its rows [y0, y1), clipped likewise
    uint32_t glyph;
    uint32_t rec;
    uint32_t fx64;     // pen_x64 mod 64
    uint32_t rgba;     // as TextInst::rgba
    uint32_t pad[2];   // as TextInst::pad
    uint32_t fy64;     // pen_y64 mod 64
    float scale;       // the placement's scale (the run's when fr_glyph_place_ex::scale is 0)
    float slant;       // k: cx = t - k * cy
    uint32_t pad2;
};
struct TextInstAffine {  // one fr_glyph_place_affine, resolved on the host: the common fields and the inverse 2 x 2 matrix
    int32_t ix;        // floor(pen_x64 / 64)
    int32_t iy;        // floor(pen_y64 / 64)
    int32_t x0, x1;    // the cell of the mapped box's four corners: columns [x0, x1), clipped to the run
    int32_t y0, y1;    // its rows [y0, y1), clipped likewise
    uint32_t glyph;
    uint32_t rec;
    uint32_t fx64;     // pen_x64 mod 64
    uint32_t rgba;     // as TextInst::rgba
    uint32_t pad[2];   // as TextInst::pad
    uint32_t fy64;     // pen_y64 mod 64
    float q00, q01;    // cx = f32(q00 * dx) + f32(q01 * dy)
    float q10, q11;    // cy = f32(q10 * dx) + f32(q11 * dy): every lane has its own ray height
    uint32_t pad2[3];
};
struct TextRun {       // == fr_text_run's geometry
    uint32_t w, h, out_x, out_y;
    float scale;
    uint32_t clear;    // an RGBA text plan's clear colour, packed as TextInst::rgba; else 0
    uint32_t pad[2];   // an sRGB text plan's linear clear colour, packed as TextInst::pad; else 0
};
struct TextTile {      // one 64 x 16 tile of a run and its instance list list[lbeg .. lend)
    uint32_t run, x0, y0, lbeg, lend;
    uint32_t pad[3];
};
// FR_TEXT_CACHE plans (fr_text_plan.cpp: text_cache_tables; the kernels of fr_text_cached.hip)
struct TextMaskCell {  // one key's mask cell: cw x ch elements of uint16_t, row-major with pitch cw, at store[base]
    TextInstEx in;     // the key's placement as an instance whose image is the whole cell: ix = -min_x, iy = max_y, x0 = y0 = 0,
                       // x1 = cw, y1 = ch, so that the mask at (X, Y) = (cell column, cell row) is the placement's own
    uint32_t base;     // first element in the store
    uint32_t pad[3];
};
struct TextMaskCellAffine {  // the same for a key of an FR_TEXT_CACHE_AFFINE plan: glyph_mask_affine_kernel reads these
    TextInstAffine in; // as TextMaskCell::in, with the key's fx64, fy64 and the inverse q00 .. q11 of the key's matrix
    uint32_t base;     // first element in the store
    uint32_t pad[3];
};
struct TextMaskTile {  // one 64 x 16 tile of a mask cell
    uint32_t cell, x0, y0, pad;
};
struct TextCachedInst {  // what a composite kernel reads of an instance: the clipped cell, the colour, and where its masks are
    int32_t x0, x1;    // as TextInst
    int32_t y0, y1;
    uint32_t rgba;     // as TextInst::rgba
    uint32_t pad[2];   // as TextInst::pad
    uint32_t base;     // TextMaskCell::base of its key's cell
    uint32_t pitch;    // cw
    int32_t c0, r0;    // the unclipped cell's origin in the run's image: the mask of pixel (X, Y) is
                       // store[base + (Y - r0) * pitch + (X - c0)]
    uint32_t pad2;
};
static_assert(sizeof(TextMaskCell) == 80 && sizeof(TextMaskTile) == 16 && sizeof(TextCachedInst) == 48, "text tables");
static_assert(sizeof(TextMaskCellAffine) == 96, "text tables");
static_assert(sizeof(TextInstEx) == 64, "text tables");
static_assert(sizeof(TextInstAffine) == 80, "text tables");
static_assert(sizeof(TextInst) == 48 && sizeof(TextRun) == 32 && sizeof(TextTile) == 32, "text tables");

constexpr int TEXT_TILE_W = 64, TEXT_TILE_H = 16, TEXT_WAVES = 4;

}  // namespace fr

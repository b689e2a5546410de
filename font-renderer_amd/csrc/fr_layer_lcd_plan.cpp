// fr_layer_lcd_plan.cpp — the host side of fr_layer_lcd (fr_layer_lcd_plan.hpp).  No HIP.
#include "fr_layer_lcd_plan.hpp"

namespace fr {

int layer_lcd_tables(const LcdIn &in, LcdTables &out)
{
    out = LcdTables{};
    constexpr uint32_t KNOWN = FR_LAYER_SRGB | FR_LCD_BGR;
    if (in.flags & ~KNOWN) return set_error(FR_E_INVALID, "unknown flag bits 0x%x", in.flags & ~KNOWN);
    if (!in.cov) return set_error(FR_E_INVALID, "cov is NULL");
    if (in.cov_stride > ((size_t)1 << 26)) return set_error(FR_E_INVALID, "cov: row pitch of %zu elements: at most 2^26", in.cov_stride);
    if (const int rc = layer_image_check("dst", in.dst, in.dst_stride)) return rc;
    if (in.cov_rows > LAYER_MAX_ROWS || in.dst_rows > LAYER_MAX_ROWS) return set_error(FR_E_UNSUPPORTED, "an image of more than 2^31 - 1 rows");
    if (in.n_blits && !in.blits) return set_error(FR_E_INVALID, "blits is NULL");
    const uint16_t *w = in.weights ? in.weights : LCD_DEFAULT_WEIGHTS;
    uint32_t sum = 0;
    for (int i = 0; i < FR_LCD_TAPS; ++i) sum += out.w[i] = w[i];
    if (sum != 256u) return set_error(FR_E_INVALID, "the weights add up to %u: must be 256", sum);

    out.clips.resize(in.n_blits);
    uint64_t n_tiles = 0;
    for (uint32_t b = 0; b < in.n_blits; ++b) {
        const fr_lcd_blit &bl = in.blits[b];
        LayerClip &c = out.clips[b];
        c = LayerClip{0, 0, 0, 0, 0, 0};
        if (!bl.w || !bl.h) continue;                          // 0 x anything: valid, and does nothing
        if ((uint64_t)bl.src_x + 3 * (uint64_t)bl.w > in.cov_stride || (uint64_t)bl.src_y + bl.h > in.cov_rows)
            return set_error(FR_E_INVALID, "blit %u: 3 x %u x %u at (%u, %u) leaves the plane of %zu x %zu", b, bl.w, bl.h, bl.src_x, bl.src_y,
                             in.cov_stride, in.cov_rows);
        c = layer_clip(0, bl.src_y, bl.w, bl.h, bl.dst_x, bl.dst_y, in.dst_stride, in.dst_rows);
        if (c.x0 < c.x1) n_tiles += layer_clip_tiles(c);
    }
    if (uint32_t p, q; layer_clips_overlap(out.clips, p, q)) return set_error(FR_E_INVALID, "blits %u and %u overlap in the destination", p, q);
    // the two images' bytes (strides <= 2^26, rows < 2^31: no overflow)
    const uintptr_t cov_end = in.cov + in.cov_stride * in.cov_rows, dst_end = in.dst + 4 * in.dst_stride * in.dst_rows;
    if (in.cov < dst_end && in.dst < cov_end) return set_error(FR_E_INVALID, "the plane and the destination overlap in memory");
    if (n_tiles > LAYER_MAX_TILES) return set_error(FR_E_UNSUPPORTED, "the blits need more than 2^22 tiles; split the call");

    const bool dvec = !(in.dst & 15u) && !(in.dst_stride % LAYER_LANE_PX), cvec = !(in.cov_stride & 3u);
    out.tiles.reserve((size_t)n_tiles);
    for (uint32_t b = 0; b < in.n_blits; ++b) {
        const LayerClip &c = out.clips[b];
        if (c.x0 >= c.x1) continue;
        const fr_lcd_blit &bl = in.blits[b];
        const uint32_t tx0 = c.x0 & ~(LAYER_LANE_PX - 1);
        // the plane element of sub-pixel 0 of column tx0: the window's pixel column c.sx of x0, less the lead
        const int32_t sq0 = (int32_t)bl.src_x + 3 * ((int32_t)c.sx - (int32_t)(c.x0 - tx0));
        // dwords of a lane's twelve bytes: 12 l and 768 per tile keep what (cov + sq0) mod 4 is, and so does a row
        const uint32_t vec = (dvec ? LAYER_DST_VEC : 0u) | (cvec && !(((int64_t)in.cov + sq0) & 3) ? LAYER_SRC_VEC : 0u);
        const uint32_t rgba = (uint32_t)bl.rgba[0] | (uint32_t)bl.rgba[1] << 8 | (uint32_t)bl.rgba[2] << 16 | (uint32_t)bl.rgba[3] << 24;
        layer_each_tile(c, [&](uint32_t x, uint32_t y) {
            out.tiles.push_back(LcdTile{x, y, c.x0, c.x1, c.y1, c.sy + (y - c.y0), sq0 + 3 * (int32_t)(x - tx0), bl.src_x, bl.src_x + 3 * bl.w, rgba, vec, 0u});
        });
    }
    return FR_OK;
}

}  // namespace fr

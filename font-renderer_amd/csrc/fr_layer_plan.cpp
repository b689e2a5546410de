// fr_layer_plan.cpp — the host side of fr_layer_over and fr_layer_unpremultiply (fr_layer_plan.hpp).  No HIP.
#include "fr_layer_plan.hpp"

#include <algorithm>

namespace fr {

int layer_tables(const LayerIn &in, LayerTables &out)
{
    out = LayerTables{};
    if (in.flags & ~(uint32_t)FR_LAYER_SRGB) return set_error(FR_E_INVALID, "unknown flag bits 0x%x", in.flags & ~(uint32_t)FR_LAYER_SRGB);
    if (const int rc = layer_image_check("src", in.src, in.src_stride)) return rc;
    if (const int rc = layer_image_check("dst", in.dst, in.dst_stride)) return rc;
    if (in.src_rows > LAYER_MAX_ROWS || in.dst_rows > LAYER_MAX_ROWS) return set_error(FR_E_UNSUPPORTED, "an image of more than 2^31 - 1 rows");
    if (in.n_blits && !in.blits) return set_error(FR_E_INVALID, "blits is NULL");
    // the two images' bytes (stride <= 2^26, rows < 2^31: no overflow)
    const uintptr_t src_end = in.src + 4 * in.src_stride * in.src_rows, dst_end = in.dst + 4 * in.dst_stride * in.dst_rows;
    if (in.src < dst_end && in.dst < src_end) return set_error(FR_E_INVALID, "the layer and the destination overlap in memory");

    const bool dvec = !(in.dst & 15u) && !(in.dst_stride % LAYER_LANE_PX), svec = !(in.src & 15u) && !(in.src_stride % LAYER_LANE_PX);
    out.clips.resize(in.n_blits);
    uint64_t n_tiles = 0;
    for (uint32_t b = 0; b < in.n_blits; ++b) {
        const fr_layer_blit &bl = in.blits[b];
        if (bl.opacity > 255u) return set_error(FR_E_INVALID, "blit %u: opacity %u above 255", b, bl.opacity);
        LayerClip &c = out.clips[b];
        c = LayerClip{0, 0, 0, 0, 0, 0};
        if (!bl.w || !bl.h) continue;                          // 0 x anything: valid, and does nothing
        if ((uint64_t)bl.src_x + bl.w > in.src_stride || (uint64_t)bl.src_y + bl.h > in.src_rows)
            return set_error(FR_E_INVALID, "blit %u: %u x %u at (%u, %u) leaves the layer of %zu x %zu", b, bl.w, bl.h, bl.src_x, bl.src_y,
                             in.src_stride, in.src_rows);
        c = layer_clip(bl.src_x, bl.src_y, bl.w, bl.h, bl.dst_x, bl.dst_y, in.dst_stride, in.dst_rows);
        if (c.x0 >= c.x1) continue;                            // nothing of it is visible: valid
        out.pixels += (uint64_t)(c.x1 - c.x0) * (uint64_t)(c.y1 - c.y0);
        if (bl.opacity == 0u) continue;                        // leaves every pixel as it is: no tile
        if (bl.opacity != 255u) out.opacity = true;
        n_tiles += layer_clip_tiles(c);
    }
    if (n_tiles > LAYER_MAX_TILES) return set_error(FR_E_UNSUPPORTED, "the blits need more than 2^22 tiles; split the call");
    // the clipped rectangles own their pixels: no two may overlap
    if (uint32_t p, q; layer_clips_overlap(out.clips, p, q)) return set_error(FR_E_INVALID, "blits %u and %u overlap in the destination", p, q);
    out.tiles.reserve((size_t)n_tiles);
    for (uint32_t b = 0; b < in.n_blits; ++b) {
        const LayerClip &c = out.clips[b];
        const uint32_t o = in.blits[b].opacity;
        if (c.x0 >= c.x1 || o == 0u) continue;
        const uint32_t tx0 = c.x0 & ~(LAYER_LANE_PX - 1);
        const int32_t sx0 = (int32_t)c.sx - (int32_t)(c.x0 - tx0);             // the layer column of tx0
        const uint32_t ov = o | (dvec ? LAYER_DST_VEC : 0u) | (svec && !(sx0 & (int32_t)(LAYER_LANE_PX - 1)) ? LAYER_SRC_VEC : 0u);
        layer_each_tile(c, [&](uint32_t x, uint32_t y) { out.tiles.push_back(LayerTile{x, y, c.x0, c.x1, c.y1, sx0 + (int32_t)(x - tx0), c.sy + (y - c.y0), ov}); });
    }
    return FR_OK;
}

int layer_window_check(uintptr_t rgba, size_t stride_px, uint32_t w, uint32_t h)
{
    if (const int rc = layer_image_check("rgba", rgba, stride_px)) return rc;
    if (w > stride_px) return set_error(FR_E_INVALID, "a window of %u pixels in rows of %zu", w, stride_px);
    if ((uint64_t)((w + LAYER_TILE_W - 1) / LAYER_TILE_W) * (((uint64_t)h + LAYER_TILE_H - 1) / LAYER_TILE_H) > LAYER_MAX_TILES)
        return set_error(FR_E_UNSUPPORTED, "the window needs more than 2^22 tiles; split the call");
    return FR_OK;
}

}  // namespace fr

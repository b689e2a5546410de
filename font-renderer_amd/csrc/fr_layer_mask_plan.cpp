// fr_layer_mask_plan.cpp — the host side of fr_layer_mask (fr_layer_mask_plan.hpp).  No HIP.
#include "fr_layer_mask_plan.hpp"

namespace fr {

int layer_mask_tables(const MaskIn &in, MaskTables &out)
{
    out = MaskTables{};
    constexpr uint32_t KNOWN = FR_LAYER_SRGB | FR_MASK_PLANE | FR_MASK_ERASE;
    if (in.flags & ~KNOWN) return set_error(FR_E_INVALID, "unknown flag bits 0x%x", in.flags & ~KNOWN);
    const bool plane = in.flags & FR_MASK_PLANE, erase = in.flags & FR_MASK_ERASE;
    if (const int rc = layer_image_check("dst", in.dst, in.dst_stride)) return rc;
    if (plane) {                                               // one byte per element: any pointer, any pitch within the limit
        if (!in.mask) return set_error(FR_E_INVALID, "mask is NULL");
        if (in.mask_stride > ((size_t)1 << 26)) return set_error(FR_E_INVALID, "mask: row pitch of %zu elements: at most 2^26", in.mask_stride);
    } else if (const int rc = layer_image_check("mask", in.mask, in.mask_stride)) {
        return rc;
    }
    if (erase && in.src) return set_error(FR_E_INVALID, "FR_MASK_ERASE takes no layer: src is not NULL");
    if (!erase && !in.src) return set_error(FR_E_INVALID, "src is NULL");
    if (!erase)
        if (const int rc = layer_image_check("src", in.src, in.src_stride)) return rc;
    if ((!erase && in.src_rows > LAYER_MAX_ROWS) || in.mask_rows > LAYER_MAX_ROWS || in.dst_rows > LAYER_MAX_ROWS)
        return set_error(FR_E_UNSUPPORTED, "an image of more than 2^31 - 1 rows");
    if (in.n_blits && !in.blits) return set_error(FR_E_INVALID, "blits is NULL");
    // the images' bytes (stride <= 2^26, rows < 2^31: no overflow)
    const uintptr_t dst_end = in.dst + 4 * in.dst_stride * in.dst_rows, mask_end = in.mask + (plane ? 1 : 4) * in.mask_stride * in.mask_rows;
    if (!erase && in.src < dst_end && in.dst < in.src + 4 * in.src_stride * in.src_rows)
        return set_error(FR_E_INVALID, "the layer and the destination overlap in memory");
    if (in.mask < dst_end && in.dst < mask_end) return set_error(FR_E_INVALID, "the mask and the destination overlap in memory");

    const bool dvec = !(in.dst & 15u) && !(in.dst_stride % LAYER_LANE_PX);
    const bool svec = !erase && !(in.src & 15u) && !(in.src_stride % LAYER_LANE_PX);
    // a layer mask: rows on the 16-byte grid; a plane: rows on the 4-byte grid once the column is added to the pointer
    const bool mrows = !(in.mask_stride % LAYER_LANE_PX) && (plane || !(in.mask & 15u));
    out.clips.resize(in.n_blits);
    out.origins.resize(in.n_blits);
    uint64_t n_tiles = 0;
    for (uint32_t b = 0; b < in.n_blits; ++b) {
        const fr_layer_mask_blit &bl = in.blits[b];
        if (bl.opacity > 255u) return set_error(FR_E_INVALID, "blit %u: opacity %u above 255", b, bl.opacity);
        if (bl.invert > 1u) return set_error(FR_E_INVALID, "blit %u: invert %u is neither 0 nor 1", b, bl.invert);
        LayerClip &c = out.clips[b];
        c = LayerClip{0, 0, 0, 0, 0, 0};
        out.origins[b] = MaskOrigin{0, 0};
        if (!bl.w || !bl.h) continue;                          // 0 x anything: valid, and does nothing
        if (!erase && ((uint64_t)bl.src_x + bl.w > in.src_stride || (uint64_t)bl.src_y + bl.h > in.src_rows))
            return set_error(FR_E_INVALID, "blit %u: %u x %u at (%u, %u) leaves the layer of %zu x %zu", b, bl.w, bl.h, bl.src_x, bl.src_y,
                             in.src_stride, in.src_rows);
        if ((uint64_t)bl.mask_x + bl.w > in.mask_stride || (uint64_t)bl.mask_y + bl.h > in.mask_rows)
            return set_error(FR_E_INVALID, "blit %u: %u x %u at (%u, %u) leaves the mask of %zu x %zu", b, bl.w, bl.h, bl.mask_x, bl.mask_y,
                             in.mask_stride, in.mask_rows);
        const uint32_t from_x = erase ? 0u : bl.src_x, from_y = erase ? 0u : bl.src_y;
        c = layer_clip(from_x, from_y, bl.w, bl.h, bl.dst_x, bl.dst_y, in.dst_stride, in.dst_rows);
        if (c.x0 >= c.x1) continue;                            // nothing of it is visible: valid
        out.origins[b] = MaskOrigin{bl.mask_x + (c.sx - from_x), bl.mask_y + (c.sy - from_y)};
        out.pixels += (uint64_t)(c.x1 - c.x0) * (uint64_t)(c.y1 - c.y0);
        if (bl.opacity == 0u) continue;                        // t = 0 everywhere: leaves every pixel as it is, no tile
        n_tiles += layer_clip_tiles(c);
    }
    if (n_tiles > LAYER_MAX_TILES) return set_error(FR_E_UNSUPPORTED, "the blits need more than 2^22 tiles; split the call");
    if (uint32_t p, q; layer_clips_overlap(out.clips, p, q)) return set_error(FR_E_INVALID, "blits %u and %u overlap in the destination", p, q);
    out.tiles.reserve((size_t)n_tiles);
    for (uint32_t b = 0; b < in.n_blits; ++b) {
        const LayerClip &c = out.clips[b];
        const MaskOrigin &g = out.origins[b];
        const uint32_t o = in.blits[b].opacity, inv = in.blits[b].invert;
        if (c.x0 >= c.x1 || o == 0u) continue;
        const uint32_t tx0 = c.x0 & ~(LAYER_LANE_PX - 1);
        const int32_t sx0 = (int32_t)c.sx - (int32_t)(c.x0 - tx0), mx0 = (int32_t)g.mx - (int32_t)(c.x0 - tx0);     // the columns of tx0
        const bool mcol = plane ? !(((int64_t)in.mask + mx0) & 3) : !(mx0 & (int32_t)(LAYER_LANE_PX - 1));
        const uint32_t ov = o | (dvec ? LAYER_DST_VEC : 0u) | (svec && !(sx0 & (int32_t)(LAYER_LANE_PX - 1)) ? LAYER_SRC_VEC : 0u) |
                            (mrows && mcol ? LAYER_MASK_VEC : 0u);
        layer_each_tile(c, [&](uint32_t x, uint32_t y) {
            out.tiles.push_back(MaskTile{x, y, c.x0, c.x1, c.y1, sx0 + (int32_t)(x - tx0), c.sy + (y - c.y0), ov, mx0 + (int32_t)(x - tx0), g.my + (y - c.y0), inv, 0u});
        });
    }
    return FR_OK;
}

}  // namespace fr

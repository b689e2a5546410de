// fr_layer_warp_plan.cpp — the host side of fr_layer_warp (fr_layer_warp_plan.hpp).  No HIP.
#include "fr_layer_warp_plan.hpp"

namespace fr {

int layer_warp_tables(const WarpIn &in, WarpTables &out)
{
    out = WarpTables{};
    if (in.flags & ~(uint32_t)FR_LAYER_SRGB) return set_error(FR_E_INVALID, "unknown flag bits 0x%x", in.flags & ~(uint32_t)FR_LAYER_SRGB);
    if (const int rc = layer_image_check("src", in.src, in.src_stride)) return rc;
    if (const int rc = layer_image_check("dst", in.dst, in.dst_stride)) return rc;
    if (in.src_rows > LAYER_MAX_ROWS || in.dst_rows > LAYER_MAX_ROWS) return set_error(FR_E_UNSUPPORTED, "an image of more than 2^31 - 1 rows");
    if (in.n_blits && !in.blits) return set_error(FR_E_INVALID, "blits is NULL");
    // the two images' bytes (stride <= 2^26, rows < 2^31: no overflow)
    const uintptr_t src_end = in.src + 4 * in.src_stride * in.src_rows, dst_end = in.dst + 4 * in.dst_stride * in.dst_rows;
    if (in.src < dst_end && in.dst < src_end) return set_error(FR_E_INVALID, "the layer and the destination overlap in memory");

    const bool dvec = !(in.dst & 15u) && !(in.dst_stride % LAYER_LANE_PX);
    out.clips.resize(in.n_blits);
    // whether blit b draws at all: a clipped rectangle that is not empty, an opacity, a window
    const auto draws = [&](uint32_t b) { return out.clips[b].x0 < out.clips[b].x1 && in.blits[b].opacity != 0u && in.blits[b].w && in.blits[b].h; };
    const auto tiles_across = [](const LayerClip &c) { return (uint64_t)((c.x1 - (c.x0 & ~(LAYER_LANE_PX - 1)) + WARP_TILE - 1) / WARP_TILE); };
    for (uint32_t b = 0; b < in.n_blits; ++b) {
        const fr_layer_warp_blit &bl = in.blits[b];
        if (bl.opacity > 255u) return set_error(FR_E_INVALID, "blit %u: opacity %u above 255", b, bl.opacity);
        if (bl.reserved != 0u) return set_error(FR_E_INVALID, "blit %u: reserved is %u, not 0", b, bl.reserved);
        if (bl.u0 > WARP_MAX_ORIGIN || bl.u0 < -WARP_MAX_ORIGIN || bl.v0 > WARP_MAX_ORIGIN || bl.v0 < -WARP_MAX_ORIGIN)
            return set_error(FR_E_INVALID, "blit %u: u0 = %lld, v0 = %lld: at most 2^47 either way", b, (long long)bl.u0, (long long)bl.v0);
        if (bl.dst_w > WARP_MAX_RECT || bl.dst_h > WARP_MAX_RECT)
            return set_error(FR_E_INVALID, "blit %u: a rectangle of %u x %u: at most 2^26 either way", b, bl.dst_w, bl.dst_h);
        if ((uint64_t)bl.src_x + bl.w > in.src_stride || (uint64_t)bl.src_y + bl.h > in.src_rows)
            return set_error(FR_E_INVALID, "blit %u: the window %u x %u at (%u, %u) leaves the layer of %zu x %zu", b, bl.w, bl.h, bl.src_x, bl.src_y,
                             in.src_stride, in.src_rows);
        LayerClip &c = out.clips[b];
        c = layer_clip(0, 0, bl.dst_w, bl.dst_h, bl.dst_x, bl.dst_y, in.dst_stride, in.dst_rows);
        if (c.x0 >= c.x1) continue;                            // nothing of it is visible, or 0 x anything: valid
        out.pixels += (uint64_t)(c.x1 - c.x0) * (uint64_t)(c.y1 - c.y0);
        if (draws(b)) out.walked += tiles_across(c) * ((c.y1 - c.y0 + WARP_TILE - 1) / WARP_TILE);
    }
    if (out.walked > LAYER_MAX_TILES) return set_error(FR_E_UNSUPPORTED, "the blits need more than 2^22 tiles; split the call");
    // the clipped rectangles own their pixels: no two may overlap
    if (uint32_t p, q; layer_clips_overlap(out.clips, p, q)) return set_error(FR_E_INVALID, "blits %u and %u overlap in the destination", p, q);
    for (uint32_t b = 0; b < in.n_blits; ++b) {
        if (!draws(b)) continue;
        const LayerClip &c = out.clips[b];
        const fr_layer_warp_blit &bl = in.blits[b];
        const uint32_t ov = bl.opacity | (dvec ? LAYER_DST_VEC : 0u);
        // a tap column i is in the window for 0 <= i < w, and a pixel at U has the columns (U - HALF) >> 16 and the next
        const int64_t u_lo = -WARP_HALF, u_hi = (int64_t)bl.w * WARP_ONE + WARP_HALF - 1, v_lo = -WARP_HALF, v_hi = (int64_t)bl.h * WARP_ONE + WARP_HALF - 1;
        bool listed = false;
        for (uint32_t y = c.y0; y < c.y1; y += WARP_TILE)
            for (uint32_t x = c.x0 & ~(LAYER_LANE_PX - 1); x < c.x1; x += WARP_TILE) {
                // the tile's pixels as rectangle pixels [X0, X1] x [Y0, Y1]
                const int64_t X0 = (int64_t)std::max(x, c.x0) - bl.dst_x, X1 = (int64_t)std::min(x + WARP_TILE, c.x1) - 1 - bl.dst_x;
                const int64_t Y0 = (int64_t)y - bl.dst_y, Y1 = (int64_t)std::min(y + WARP_TILE, c.y1) - 1 - bl.dst_y;
                int64_t ulo, uhi, vlo, vhi;
                warp_extremes(bl.u0, bl.ux, bl.uy, X0, X1, Y0, Y1, ulo, uhi);
                warp_extremes(bl.v0, bl.vx, bl.vy, X0, X1, Y0, Y1, vlo, vhi);
                if (uhi < u_lo || ulo > u_hi || vhi < v_lo || vlo > v_hi) continue;     // no tap of the tile can be in the window
                WarpTile t{};
                t.x = x, t.y = y, t.x0 = c.x0, t.x1 = c.x1, t.y1 = c.y1, t.ov = ov;
                t.wx = bl.src_x, t.wy = bl.src_y, t.ww = bl.w, t.wh = bl.h;
                t.U = bl.u0 + ((int64_t)x - bl.dst_x) * bl.ux + Y0 * bl.uy;
                t.V = bl.v0 + ((int64_t)x - bl.dst_x) * bl.vx + Y0 * bl.vy;
                t.ux = bl.ux, t.uy = bl.uy, t.vx = bl.vx, t.vy = bl.vy;
                t.i0 = (uint32_t)std::max<int64_t>((ulo - WARP_HALF) >> 16, 0);
                t.i1 = (uint32_t)std::min<int64_t>(((uhi - WARP_HALF) >> 16) + 1, (int64_t)bl.w - 1);
                t.j0 = (uint32_t)std::max<int64_t>((vlo - WARP_HALF) >> 16, 0);
                t.j1 = (uint32_t)std::min<int64_t>(((vhi - WARP_HALF) >> 16) + 1, (int64_t)bl.h - 1);
                out.tiles.push_back(t);
                listed = true;
            }
        if (listed && bl.opacity != 255u) out.opacity = true;
    }
    return FR_OK;
}

}  // namespace fr

// fr_layer_paint_plan.cpp — the host side of fr_layer_paint (fr_layer_paint_plan.hpp).  No HIP.
#include "fr_layer_paint_plan.hpp"

#include <algorithm>
#include <cstdlib>
#include <initializer_list>

namespace fr {

int64_t paint_rdiv(__int128 n, int64_t d)
{
    const __int128 num = 2 * n + d, den = 2 * (__int128)d;
    __int128 q = num / den;
    if (num % den < 0) --q;                                    // C++ truncates: floor for a negative numerator
    return (int64_t)q;
}

namespace {

// G of the header: the gradient at q = 64 k + 32, interpolated on the stops' stored bytes
void colour_table(const fr_layer_paint_params &p, uint32_t *G)
{
    const uint32_t n = p.n_stops;
    for (uint32_t k = 0; k < PAINT_TABLE; ++k) {
        const uint32_t q = 64u * k + 32u;
        uint8_t c[4];
        if (q < p.stops[0].offset || q >= p.stops[n - 1].offset) {
            const fr_gradient_stop &s = p.stops[q < p.stops[0].offset ? 0 : n - 1];
            for (int j = 0; j < 4; ++j) c[j] = s.rgba[j];
        } else {
            uint32_t i = 0;                                    // the largest index with off[i] <= q; i + 1 < n, and wd > 0
            while (i + 2 < n && p.stops[i + 1].offset <= q) ++i;
            const fr_gradient_stop &a = p.stops[i], &b = p.stops[i + 1];
            const uint32_t wd = b.offset - a.offset, f = q - a.offset;
            for (int j = 0; j < 4; ++j) c[j] = (uint8_t)((a.rgba[j] * (wd - f) + b.rgba[j] * f + wd / 2) / wd);
        }
        G[k] = (uint32_t)c[0] | (uint32_t)c[1] << 8 | (uint32_t)c[2] << 16 | (uint32_t)c[3] << 24;
    }
}

}  // namespace

int layer_paint_plan(const PaintIn &in, PaintPlan &out)
{
    out.nothing = true;
    if (in.flags & ~(uint32_t)FR_LAYER_SRGB) return set_error(FR_E_INVALID, "unknown flag bits 0x%x", in.flags & ~(uint32_t)FR_LAYER_SRGB);
    if (const int rc = layer_image_check("dst", in.dst, in.dst_stride)) return rc;
    if (in.src) {
        if (const int rc = layer_image_check("src", in.src, in.src_stride)) return rc;
    } else if (in.src_stride || in.src_rows) {
        return set_error(FR_E_INVALID, "src is NULL (full coverage) with a layer of %zu x %zu", in.src_stride, in.src_rows);
    }
    if (in.src_rows > LAYER_MAX_ROWS || in.dst_rows > LAYER_MAX_ROWS) return set_error(FR_E_UNSUPPORTED, "an image of more than 2^31 - 1 rows");
    if (!in.paint) return set_error(FR_E_INVALID, "paint is NULL");
    const fr_layer_paint_params &p = *in.paint;
    if (in.src) {
        if (p.w && p.h && ((uint64_t)p.src_x + p.w > in.src_stride || (uint64_t)p.src_y + p.h > in.src_rows))
            return set_error(FR_E_INVALID, "the window of %u x %u at (%u, %u) leaves the layer of %zu x %zu", p.w, p.h, p.src_x, p.src_y, in.src_stride, in.src_rows);
    } else if (p.src_x || p.src_y) {
        return set_error(FR_E_INVALID, "src is NULL (full coverage) with a window at (%u, %u)", p.src_x, p.src_y);
    }
    if (p.kind > FR_GRADIENT_RADIAL) return set_error(FR_E_INVALID, "unknown gradient kind %u", p.kind);
    if (p.spread > FR_SPREAD_REFLECT) return set_error(FR_E_INVALID, "unknown spread %u", p.spread);
    if (p.n_stops < 1 || p.n_stops > FR_GRADIENT_MAX_STOPS) return set_error(FR_E_INVALID, "%u stops: 1 .. 8", p.n_stops);
    for (uint32_t i = 0; i < p.n_stops; ++i) {
        if (p.stops[i].offset > 65536u) return set_error(FR_E_INVALID, "stop %u: offset %u above 65536", i, p.stops[i].offset);
        if (i && p.stops[i].offset < p.stops[i - 1].offset) return set_error(FR_E_INVALID, "stop %u: offset %u below the stop before it", i, p.stops[i].offset);
    }
    const bool radial = p.kind == FR_GRADIENT_RADIAL;
    const int64_t dx = (int64_t)p.x1 - p.x0, dy = (int64_t)p.y1 - p.y0, L2 = dx * dx + dy * dy;    // (below 2^65 / 2: no overflow)
    if (!radial && L2 == 0) return set_error(FR_E_INVALID, "a linear gradient of length 0");
    if (radial && p.x1 <= 0) return set_error(FR_E_INVALID, "a radial gradient of radius %d", p.x1);
    if (radial && p.y1 != 0) return set_error(FR_E_INVALID, "a radial gradient with y1 = %d: must be 0", p.y1);
    if (in.src) {
        // the two images' bytes (stride <= 2^26, rows < 2^31: no overflow)
        const uintptr_t src_end = in.src + 4 * in.src_stride * in.src_rows, dst_end = in.dst + 4 * in.dst_stride * in.dst_rows;
        if (in.src < dst_end && in.dst < src_end) return set_error(FR_E_INVALID, "the layer and the destination overlap in memory");
    }
    for (const int32_t v : {p.x0, p.y0, p.x1, p.y1})
        if (v > PAINT_MAX_COORD || v < -PAINT_MAX_COORD) return set_error(FR_E_UNSUPPORTED, "geometry value %d beyond 2^26 in 1/64 pixel", v);
    if (!radial && L2 < PAINT_MIN_L2) return set_error(FR_E_UNSUPPORTED, "a linear gradient shorter than one pixel");
    if (radial && p.x1 < PAINT_MIN_R) return set_error(FR_E_UNSUPPORTED, "a radial gradient of a radius below one pixel");

    // clip to [0, dst_stride) x [0, dst_rows), as a blit of fr_layer_over
    const int64_t x0 = std::max<int64_t>(p.dst_x, 0), y0 = std::max<int64_t>(p.dst_y, 0);
    const int64_t x1 = std::min<int64_t>((int64_t)p.dst_x + p.w, (int64_t)in.dst_stride);
    const int64_t y1 = std::min<int64_t>((int64_t)p.dst_y + p.h, (int64_t)in.dst_rows);
    const bool drawn = p.w && p.h && x0 < x1 && y0 < y1;
    if (drawn && radial)
        for (const int64_t X : {x0, x1 - 1})
            for (const int64_t Y : {y0, y1 - 1}) {
                const int64_t ddx = 64 * X + 32 - p.x0, ddy = 64 * Y + 32 - p.y0;
                if (std::max(std::abs(ddx), std::abs(ddy)) >= PAINT_MAX_DD)
                    return set_error(FR_E_UNSUPPORTED, "pixel (%lld, %lld) is 2^27 / 64 pixels or more from the radial centre", (long long)X, (long long)Y);
            }
    if (!drawn) return FR_OK;
    const uint32_t tx0 = (uint32_t)x0 & ~(LAYER_LANE_PX - 1);
    const uint64_t nx = ((uint64_t)x1 - tx0 + LAYER_TILE_W - 1) / LAYER_TILE_W, ny = ((uint64_t)(y1 - y0) + LAYER_TILE_H - 1) / LAYER_TILE_H;
    if (nx * ny > LAYER_MAX_TILES) return set_error(FR_E_UNSUPPORTED, "the rectangle needs more than 2^22 tiles; split the call");

    out.nothing = false;
    out.x0 = (uint32_t)x0, out.y0 = (uint32_t)y0, out.x1 = (uint32_t)x1, out.y1 = (uint32_t)y1;
    out.sx = (uint32_t)(p.src_x + (x0 - p.dst_x)), out.sy = (uint32_t)(p.src_y + (y0 - p.dst_y));
    out.tx0 = tx0, out.tiles_x = (uint32_t)nx, out.tiles_y = (uint32_t)ny;
    out.sx0 = (int32_t)out.sx - (int32_t)((uint32_t)x0 - tx0);
    out.dst_vec = !(in.dst & 15u) && !(in.dst_stride % LAYER_LANE_PX);
    out.src_vec = in.src && !(in.src & 15u) && !(in.src_stride % LAYER_LANE_PX) && !(out.sx0 & (int32_t)(LAYER_LANE_PX - 1));
    if (radial) {
        out.c[0] = p.x0, out.c[1] = p.y0, out.c[2] = paint_rdiv((__int128)1 << 60, p.x1);
    } else {
        const __int128 one = (__int128)1 << 32;
        out.c[0] = paint_rdiv(((__int128)(32 - (int64_t)p.x0) * dx + (__int128)(32 - (int64_t)p.y0) * dy) * one, L2);
        out.c[1] = paint_rdiv(64 * (__int128)dx * one, L2);
        out.c[2] = paint_rdiv(64 * (__int128)dy * one, L2);
    }
    colour_table(p, out.table);
    return FR_OK;
}

}  // namespace fr

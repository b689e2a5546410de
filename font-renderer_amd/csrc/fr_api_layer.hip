// fr_api_layer.hip — C ABI (include/fr_raster.h): fr_layer_over, fr_layer_unpremultiply, fr_layer_shadow, fr_layer_outline,
// fr_layer_rects, fr_layer_paint, fr_layer_lcd, fr_layer_mask, fr_layer_warp and fr_layer_blend.  The checks, the clipping and the tile table are
// fr_layer_plan.cpp's (fr_layer_blend's too, behind its mode check: fr_layer_blend_math.hpp), the shadow's stages fr_layer_shadow_plan.cpp's, the outline's rectangles and weights
// fr_layer_outline_plan.cpp's, the rectangles' tables fr_layer_rects_plan.cpp's, the gradient's coefficients and colour
// table fr_layer_paint_plan.cpp's, the sub-pixel blits' tiles fr_layer_lcd_plan.cpp's, the masked blits' tiles
// fr_layer_mask_plan.cpp's, the warped blits' culled tiles fr_layer_warp_plan.cpp's; this unit stages the tables, keeps the shadow's planes and launches the kernels of
// fr_layer.hip, fr_layer_shadow.hip, fr_layer_outline.hip, fr_layer_rects.hip, fr_layer_paint.hip, fr_layer_lcd.hip,
// fr_layer_mask.hip, fr_layer_warp.hip and fr_layer_blend.hip.
#include "fr_internal.hpp"
#include "fr_layer.hpp"
#include "fr_layer_blend.hpp"
#include "fr_layer_lcd.hpp"
#include "fr_layer_mask.hpp"
#include "fr_layer_outline.hpp"
#include "fr_layer_paint.hpp"
#include "fr_layer_rects.hpp"
#include "fr_layer_shadow.hpp"
#include "fr_layer_warp.hpp"

#include <algorithm>
#include <cstring>
#include <new>

// Room for n units of 16 bytes in the context's tables: pinned staging on the host, which the device reads, and its DevBuf on
// the device, grown on demand.  The earlier tables may still be read by a kernel in flight, so growing waits for the stream.
static int layer_table_room(fr_ctx *ctx, size_t n)
{
    if (n <= ctx->layer_cap) return FR_OK;
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (ctx->layer_stage) { (void)hipHostFree(ctx->layer_stage); ctx->layer_stage = nullptr; }
    ctx->layer_tab.reset();
    ctx->layer_cap = 0;
    const size_t cap = std::max<size_t>(n + n / 2, 2048);
    hipError_t e = hipHostMalloc(reinterpret_cast<void **>(&ctx->layer_stage), cap * sizeof(uint4), hipHostMallocDefault);
    if (e != hipSuccess) { ctx->layer_stage = nullptr; return hip_fail(e, "hipHostMalloc(&ctx->layer_stage, cap)"); }
    ctx->layer_tab.alloc(e, cap * sizeof(uint4));
    if (e != hipSuccess) return hip_fail(e, "hipMalloc(&ctx->layer_tab, cap)");
    ctx->layer_cap = cap;
    return FR_OK;
}

// The tables of one call, `units` units of 16 bytes that `fill` writes into the staging, brought into the context's device
// copy in stream order; -> that copy in *table.  A kernel launched on the stream after this reads the call's own tables
// even while an earlier call's kernels are still in flight.
template <class FILL>
static int layer_tables_to_device(fr_ctx *ctx, size_t units, const uint4 **table, FILL fill)
{
    // the tables of the call before this one have left the staging (layer_table_kernel reads it in stream order)
    if (ctx->layer_ev) HIP_TRY(hipEventSynchronize(ctx->layer_ev));
    else HIP_TRY(hipEventCreateWithFlags(&ctx->layer_ev, hipEventDisableTiming));
    if (const int rc = layer_table_room(ctx, units)) return rc;
    fill(ctx->layer_stage);
    HIP_TRY(fr::launch_layer_table(ctx->layer_stage, ctx->layer_tab.get(), (uint32_t)units, ctx->stream));
    HIP_TRY(hipEventRecord(ctx->layer_ev, ctx->stream));
    *table = ctx->layer_tab.get();
    return FR_OK;
}

// Room for need[i] bytes in plane i of the context.  A stage in flight may still use an earlier plane, so growing waits for
// the stream, once, as the tile table does; a plane that cannot grow stays as it was.
static int shadow_plane_room(fr_ctx *ctx, const uint64_t need[2])
{
    if (need[0] <= ctx->shadow_cap[0] && need[1] <= ctx->shadow_cap[1]) return FR_OK;
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    for (int i = 0; i < 2; ++i) {
        if (need[i] <= ctx->shadow_cap[i]) continue;
        const size_t cap = (size_t)(need[i] + need[i] / 4);
        hipError_t e = hipSuccess;
        DevBuf<unsigned char> grown;
        grown.alloc(e, cap);
        if (e != hipSuccess) return hip_fail(e, "hipMalloc(&ctx->shadow_plane, cap)");
        ctx->shadow_plane[i] = std::move(grown);
        ctx->shadow_cap[i] = cap;
    }
    return FR_OK;
}

extern "C" {

int fr_layer_over(fr_ctx *ctx, const void *src_dev, size_t src_stride_px, size_t src_rows, void *dst_dev, size_t dst_stride_px,
                  size_t dst_rows, const fr_layer_blit *blits, uint32_t n_blits, uint32_t flags)
{
    if (!ctx) return fail(FR_E_INVALID, "fr_layer_over: ctx is NULL");
    fr::LayerTables t;
    try {
        const fr::LayerIn in{(uintptr_t)src_dev, (uintptr_t)dst_dev, src_stride_px, src_rows, dst_stride_px, dst_rows, blits, n_blits, flags};
        if (const int rc = fr::layer_tables(in, t)) return rc;
    } catch (const std::bad_alloc &) {
        return fail(FR_E_NOMEM, "fr_layer_over: host allocation");
    }
    const size_t n = t.tiles.size();
    if (!n) return FR_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    static_assert(sizeof(fr::LayerTile) == 2 * sizeof(uint4), "a tile is two units of the staging");
    const uint4 *tab = nullptr;
    if (const int rc = layer_tables_to_device(ctx, 2 * n, &tab, [&](uint4 *to) { memcpy(to, t.tiles.data(), n * sizeof(fr::LayerTile)); })) return rc;
    const fr::LayerArgs a{reinterpret_cast<const fr::LayerTile *>(tab), static_cast<const uint32_t *>(src_dev), static_cast<uint32_t *>(dst_dev), src_stride_px, dst_stride_px};
    HIP_TRY(fr::launch_layer_over((flags & FR_LAYER_SRGB) != 0, t.opacity, (uint32_t)n, a, ctx->stream));
    return FR_OK;
}

int fr_layer_unpremultiply(fr_ctx *ctx, void *rgba_dev, size_t stride_px, uint32_t w, uint32_t h, int srgb)
{
    if (!ctx) return fail(FR_E_INVALID, "fr_layer_unpremultiply: ctx is NULL");
    if (const int rc = fr::layer_window_check((uintptr_t)rgba_dev, stride_px, w, h)) return rc;
    if (!w || !h) return FR_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(fr::launch_layer_unpremultiply(srgb != 0, static_cast<uint32_t *>(rgba_dev), stride_px, w, h, ctx->stream));
    return FR_OK;
}

int fr_layer_shadow(fr_ctx *ctx, const void *src_dev, size_t src_stride_px, size_t src_rows, void *dst_dev, size_t dst_stride_px,
                    size_t dst_rows, const fr_layer_shadow_params *shadow, uint32_t flags)
{
    if (!ctx) return fail(FR_E_INVALID, "fr_layer_shadow: ctx is NULL");
    fr::ShadowPlan p;
    try {
        const fr::ShadowIn in{(uintptr_t)src_dev, (uintptr_t)dst_dev, src_stride_px, src_rows, dst_stride_px, dst_rows, shadow, flags};
        if (const int rc = fr::shadow_plan(in, p)) return rc;
    } catch (const std::bad_alloc &) {
        return fail(FR_E_NOMEM, "fr_layer_shadow: host allocation");
    }
    if (p.nothing) return FR_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    if (const int rc = shadow_plane_room(ctx, p.plane_bytes)) return rc;
    const fr_layer_shadow_params &s = *shadow;
    const size_t n = p.stages.size();
    // the input of the stage at hand: the window of the layer, then the plane of the stage before
    fr::ShadowArgs a{};
    a.in = src_dev;                                             // (an input without extent is never loaded from)
    if (!p.zeros) {
        a.in = static_cast<const uint32_t *>(src_dev) + ((uint64_t)s.src_y * src_stride_px + s.src_x);
        a.in_w = s.w;
        a.in_h = s.h;
    }
    a.in_pitch = src_stride_px;
    fr::ShadowRect in_rect{0, 0, 0, 0};                         // its first pixel in window coordinates
    for (size_t k = 0; k < std::max<size_t>(n, 1); ++k) {
        const bool last = k + 1 >= n;
        fr::ShadowOp op = fr::SHADOW_OP_NONE;
        if (n) {
            const fr::ShadowStage &st = p.stages[k];
            op = st.kind == fr::SHADOW_SPREAD ? fr::SHADOW_OP_MAX : fr::SHADOW_OP_BOX;
            a.radius = st.radius;
            a.recip_m = st.recip.m;
            a.recip_shift = st.recip.shift;
            a.half_w = (2 * st.radius + 1) * (2 * st.radius + 1) / 2;
        }
        if (last) {                                            // the whole destination rectangle, tinted
            uint32_t *first = static_cast<uint32_t *>(dst_dev) + ((uint64_t)s.dst_y * dst_stride_px + s.dst_x);
            a.out = first;
            a.out_pitch = dst_stride_px;
            a.out_w = s.dst_w;
            a.out_h = s.dst_h;
            a.off_x = p.want.x0 - in_rect.x0;
            a.off_y = p.want.y0 - in_rect.y0;
            a.vec = dst_stride_px % 4 == 0;
            a.lead = a.vec ? (uint32_t)(((uintptr_t)first >> 2) & 3u) : 0u;
            a.rgba = (uint32_t)s.rgba[0] | (uint32_t)s.rgba[1] << 8 | (uint32_t)s.rgba[2] << 16 | (uint32_t)s.rgba[3] << 24;
            a.srgb = flags & FR_LAYER_SRGB;
        } else {
            const fr::ShadowStage &st = p.stages[k];
            a.out = ctx->shadow_plane[k & 1].get();
            a.out_pitch = st.pitch;
            a.out_w = (uint32_t)st.out.w();
            a.out_h = (uint32_t)st.out.h();
            a.off_x = st.out.x0 - in_rect.x0;
            a.off_y = st.out.y0 - in_rect.y0;
        }
        HIP_TRY(fr::launch_layer_shadow(k == 0, op, last, a, ctx->stream));
        if (!last) {
            const fr::ShadowStage &st = p.stages[k];
            a.in = a.out;
            a.in_pitch = st.pitch;
            a.in_w = a.out_w;
            a.in_h = a.out_h;
            in_rect = st.out;
        }
    }
    return FR_OK;
}

int fr_layer_outline(fr_ctx *ctx, const void *src_dev, size_t src_stride_px, size_t src_rows, void *dst_dev, size_t dst_stride_px,
                     size_t dst_rows, const fr_layer_outline_params *outline, uint32_t flags)
{
    if (!ctx) return fail(FR_E_INVALID, "fr_layer_outline: ctx is NULL");
    fr::OutlinePlan p;
    try {
        const fr::OutlineIn in{(uintptr_t)src_dev, (uintptr_t)dst_dev, src_stride_px, src_rows, dst_stride_px, dst_rows, outline, flags};
        if (const int rc = fr::outline_plan(in, p)) return rc;
    } catch (const std::bad_alloc &) {
        return fail(FR_E_NOMEM, "fr_layer_outline: host allocation");
    }
    if (p.nothing) return FR_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    const fr_layer_outline_params &s = *outline;
    uint32_t *const first = static_cast<uint32_t *>(dst_dev) + ((uint64_t)s.dst_y * dst_stride_px + s.dst_x);
    const uint32_t rgba = (uint32_t)s.rgba[0] | (uint32_t)s.rgba[1] << 8 | (uint32_t)s.rgba[2] << 16 | (uint32_t)s.rgba[3] << 24;
    if (p.zeros) {                                              // the shadow's extract-and-tint over an input without extent
        fr::ShadowArgs z{};
        z.in = src_dev;
        z.in_pitch = src_stride_px;
        z.out = first;
        z.out_pitch = dst_stride_px;
        z.out_w = s.dst_w;
        z.out_h = s.dst_h;
        z.vec = p.vec;
        z.lead = p.lead;
        z.rgba = rgba;
        z.srgb = flags & FR_LAYER_SRGB;
        HIP_TRY(fr::launch_layer_shadow(true, fr::SHADOW_OP_NONE, true, z, ctx->stream));
        return FR_OK;
    }
    const uint4 *tab = nullptr;
    if (const int rc = layer_tables_to_device(ctx, p.table.units(), &tab, [&](uint4 *to) { memcpy(to, p.table.packed.data(), p.table.packed.size() * sizeof(uint32_t)); }))
        return rc;
    fr::OutlineArgs a{};
    a.in = static_cast<const uint32_t *>(src_dev) + ((uint64_t)s.src_y * src_stride_px + s.src_x);
    a.out = first;
    a.table = tab;
    a.units = (uint32_t)p.table.units();
    a.in_pitch = src_stride_px;
    a.out_pitch = dst_stride_px;
    a.off_x = p.want.x0;
    a.off_y = p.want.y0;
    a.in_w = s.w;
    a.in_h = s.h;
    a.out_w = s.dst_w;
    a.out_h = s.dst_h;
    a.live_x0 = (uint32_t)(p.live.x0 - p.want.x0);
    a.live_y0 = (uint32_t)(p.live.y0 - p.want.y0);
    a.live_x1 = (uint32_t)(p.live.x1 - p.want.x0);
    a.live_y1 = (uint32_t)(p.live.y1 - p.want.y0);
    a.reach = p.table.reach;
    a.levels = p.table.levels;
    a.lead = p.lead;
    a.vec = p.vec;
    a.rgba = rgba;
    a.srgb = flags & FR_LAYER_SRGB;
    a.tiles_x = (uint32_t)p.tiles_x;
    HIP_TRY(fr::launch_layer_outline(s.kind, (uint32_t)(p.tiles_x * p.tiles_y), a, ctx->stream));
    return FR_OK;
}

int fr_layer_rects(fr_ctx *ctx, void *dst_dev, size_t dst_stride_px, size_t dst_rows, const fr_layer_rect *rects, uint32_t n_rects,
                   uint32_t flags)
{
    if (!ctx) return fail(FR_E_INVALID, "fr_layer_rects: ctx is NULL");
    fr::RectsTables t;
    try {
        const fr::RectsIn in{(uintptr_t)dst_dev, dst_stride_px, dst_rows, rects, n_rects, flags};
        if (const int rc = fr::layer_rects_tables(in, t)) return rc;
    } catch (const std::bad_alloc &) {
        return fail(FR_E_NOMEM, "fr_layer_rects: host allocation");
    }
    const size_t n = t.tiles.size();
    if (!n) return FR_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    // the three tables back to back, each from a 16-byte boundary: tiles (one unit each), the list, the records (two each)
    const size_t list_at = n, recs_at = list_at + (t.list.size() + 3) / 4, units = recs_at + 2 * t.recs.size();
    const uint4 *tab = nullptr;
    if (const int rc = layer_tables_to_device(ctx, units, &tab, [&](uint4 *to) {
            memcpy(to, t.tiles.data(), n * sizeof(fr::RectTile));
            to[recs_at - 1] = make_uint4(0u, 0u, 0u, 0u);       // (the list's last unit may be part-filled)
            memcpy(to + list_at, t.list.data(), t.list.size() * sizeof(uint32_t));
            memcpy(to + recs_at, t.recs.data(), t.recs.size() * sizeof(fr::RectRec));
        })) return rc;
    const fr::RectsArgs a{reinterpret_cast<const fr::RectTile *>(tab), reinterpret_cast<const uint32_t *>(tab + list_at),
                          reinterpret_cast<const fr::RectRec *>(tab + recs_at), static_cast<uint32_t *>(dst_dev), dst_stride_px, t.dst_vec ? 1u : 0u};
    HIP_TRY(fr::launch_layer_rects((flags & FR_LAYER_SRGB) != 0, (uint32_t)n, a, ctx->stream));
    return FR_OK;
}

int fr_layer_paint(fr_ctx *ctx, const void *src_dev, size_t src_stride_px, size_t src_rows, void *dst_dev, size_t dst_stride_px,
                   size_t dst_rows, const fr_layer_paint_params *paint, uint32_t flags)
{
    if (!ctx) return fail(FR_E_INVALID, "fr_layer_paint: ctx is NULL");
    fr::PaintPlan p;
    const fr::PaintIn in{(uintptr_t)src_dev, (uintptr_t)dst_dev, src_stride_px, src_rows, dst_stride_px, dst_rows, paint, flags};
    if (const int rc = fr::layer_paint_plan(in, p)) return rc;
    if (p.nothing) return FR_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    // the colour table goes through the staging; the clipped rectangle and the three coefficients are kernel arguments
    static_assert(sizeof p.table == fr::PAINT_TABLE / 4 * sizeof(uint4), "the table in units of the staging");
    const uint4 *tab = nullptr;
    if (const int rc = layer_tables_to_device(ctx, fr::PAINT_TABLE / 4, &tab, [&](uint4 *to) { memcpy(to, p.table, sizeof p.table); })) return rc;
    const fr::PaintArgs a{reinterpret_cast<const uint32_t *>(tab), static_cast<const uint32_t *>(src_dev), static_cast<uint32_t *>(dst_dev),
                          src_stride_px, dst_stride_px, p.x0, p.x1, p.y0, p.y1, p.tx0, p.tiles_x, p.sx0, p.sy,
                          (p.dst_vec ? fr::LAYER_DST_VEC : 0u) | (p.src_vec ? fr::LAYER_SRC_VEC : 0u), paint->spread, {p.c[0], p.c[1], p.c[2]}};
    HIP_TRY(fr::launch_layer_paint((flags & FR_LAYER_SRGB) != 0, paint->kind == FR_GRADIENT_RADIAL, p.tiles_x * p.tiles_y, a, ctx->stream));
    return FR_OK;
}

int fr_layer_lcd(fr_ctx *ctx, const void *cov_dev, size_t cov_stride, size_t cov_rows, void *dst_dev, size_t dst_stride_px, size_t dst_rows,
                 const fr_lcd_blit *blits, uint32_t n_blits, const uint16_t *weights, uint32_t flags)
{
    if (!ctx) return fail(FR_E_INVALID, "fr_layer_lcd: ctx is NULL");
    fr::LcdTables t;
    try {
        const fr::LcdIn in{(uintptr_t)cov_dev, (uintptr_t)dst_dev, cov_stride, cov_rows, dst_stride_px, dst_rows, blits, n_blits, weights, flags};
        if (const int rc = fr::layer_lcd_tables(in, t)) return rc;
    } catch (const std::bad_alloc &) {
        return fail(FR_E_NOMEM, "fr_layer_lcd: host allocation");
    }
    const size_t n = t.tiles.size();
    if (!n) return FR_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    // the tiles, each with its blit's colour and window, go through the staging; the filter is a kernel argument
    static_assert(sizeof(fr::LcdTile) == 3 * sizeof(uint4), "a tile is three units of the staging");
    const uint4 *tab = nullptr;
    if (const int rc = layer_tables_to_device(ctx, 3 * n, &tab, [&](uint4 *to) { memcpy(to, t.tiles.data(), n * sizeof(fr::LcdTile)); })) return rc;
    const fr::LcdArgs a{reinterpret_cast<const fr::LcdTile *>(tab), static_cast<const uint8_t *>(cov_dev), static_cast<uint32_t *>(dst_dev), cov_stride, dst_stride_px,
                        {t.w[0], t.w[1], t.w[2], t.w[3], t.w[4]}, (flags & FR_LCD_BGR) ? 1u : 0u};
    HIP_TRY(fr::launch_layer_lcd((flags & FR_LAYER_SRGB) != 0, (uint32_t)n, a, ctx->stream));
    return FR_OK;
}

int fr_layer_mask(fr_ctx *ctx, const void *src_dev, size_t src_stride_px, size_t src_rows, const void *mask_dev, size_t mask_stride, size_t mask_rows,
                  void *dst_dev, size_t dst_stride_px, size_t dst_rows, const fr_layer_mask_blit *blits, uint32_t n_blits, uint32_t flags)
{
    if (!ctx) return fail(FR_E_INVALID, "fr_layer_mask: ctx is NULL");
    fr::MaskTables t;
    try {
        const fr::MaskIn in{(uintptr_t)src_dev, (uintptr_t)mask_dev, (uintptr_t)dst_dev, src_stride_px, src_rows, mask_stride, mask_rows, dst_stride_px, dst_rows, blits, n_blits, flags};
        if (const int rc = fr::layer_mask_tables(in, t)) return rc;
    } catch (const std::bad_alloc &) {
        return fail(FR_E_NOMEM, "fr_layer_mask: host allocation");
    }
    const size_t n = t.tiles.size();
    if (!n) return FR_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    static_assert(sizeof(fr::MaskTile) == 3 * sizeof(uint4), "a tile is three units of the staging");
    const uint4 *tab = nullptr;
    if (const int rc = layer_tables_to_device(ctx, 3 * n, &tab, [&](uint4 *to) { memcpy(to, t.tiles.data(), n * sizeof(fr::MaskTile)); })) return rc;
    const fr::MaskArgs a{reinterpret_cast<const fr::MaskTile *>(tab), static_cast<const uint32_t *>(src_dev), mask_dev, static_cast<uint32_t *>(dst_dev),
                         src_stride_px, mask_stride, dst_stride_px};
    HIP_TRY(fr::launch_layer_mask((flags & FR_LAYER_SRGB) != 0, (flags & FR_MASK_PLANE) != 0, (flags & FR_MASK_ERASE) != 0, (uint32_t)n, a, ctx->stream));
    return FR_OK;
}

int fr_layer_warp(fr_ctx *ctx, const void *src_dev, size_t src_stride_px, size_t src_rows, void *dst_dev, size_t dst_stride_px,
                  size_t dst_rows, const fr_layer_warp_blit *blits, uint32_t n_blits, uint32_t flags)
{
    if (!ctx) return fail(FR_E_INVALID, "fr_layer_warp: ctx is NULL");
    fr::WarpTables t;
    try {
        const fr::WarpIn in{(uintptr_t)src_dev, (uintptr_t)dst_dev, src_stride_px, src_rows, dst_stride_px, dst_rows, blits, n_blits, flags};
        if (const int rc = fr::layer_warp_tables(in, t)) return rc;
    } catch (const std::bad_alloc &) {
        return fail(FR_E_NOMEM, "fr_layer_warp: host allocation");
    }
    const size_t n = t.tiles.size();
    if (!n) return FR_OK;                                       // no tap of any tile reaches a window
    HIP_TRY(hipSetDevice(ctx->device));
    static_assert(sizeof(fr::WarpTile) == 6 * sizeof(uint4), "a tile is six units of the staging");
    const uint4 *tab = nullptr;
    if (const int rc = layer_tables_to_device(ctx, 6 * n, &tab, [&](uint4 *to) { memcpy(to, t.tiles.data(), n * sizeof(fr::WarpTile)); })) return rc;
    const fr::WarpArgs a{reinterpret_cast<const fr::WarpTile *>(tab), static_cast<const uint32_t *>(src_dev), static_cast<uint32_t *>(dst_dev), src_stride_px, dst_stride_px};
    HIP_TRY(fr::launch_layer_warp((flags & FR_LAYER_SRGB) != 0, t.opacity, (uint32_t)n, a, ctx->stream));
    return FR_OK;
}

int fr_layer_blend(fr_ctx *ctx, const void *src_dev, size_t src_stride_px, size_t src_rows, void *dst_dev, size_t dst_stride_px,
                   size_t dst_rows, const fr_layer_blit *blits, uint32_t n_blits, uint32_t mode, uint32_t flags)
{
    if (!ctx) return fail(FR_E_INVALID, "fr_layer_blend: ctx is NULL");
    fr::LayerTables t;
    try {
        const fr::LayerIn in{(uintptr_t)src_dev, (uintptr_t)dst_dev, src_stride_px, src_rows, dst_stride_px, dst_rows, blits, n_blits, flags};
        if (const int rc = fr::layer_blend_tables(in, mode, t)) return rc;
    } catch (const std::bad_alloc &) {
        return fail(FR_E_NOMEM, "fr_layer_blend: host allocation");
    }
    const size_t n = t.tiles.size();
    if (!n) return FR_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    const uint4 *tab = nullptr;
    if (const int rc = layer_tables_to_device(ctx, 2 * n, &tab, [&](uint4 *to) { memcpy(to, t.tiles.data(), n * sizeof(fr::LayerTile)); })) return rc;
    const fr::LayerArgs a{reinterpret_cast<const fr::LayerTile *>(tab), static_cast<const uint32_t *>(src_dev), static_cast<uint32_t *>(dst_dev), src_stride_px, dst_stride_px};
    HIP_TRY(fr::launch_layer_blend((flags & FR_LAYER_SRGB) != 0, mode, t.opacity, (uint32_t)n, a, ctx->stream));
    return FR_OK;
}

}  // extern "C"

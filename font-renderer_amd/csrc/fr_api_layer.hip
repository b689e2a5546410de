// fr_api_layer.hip — C ABI (include/fr_raster.h): fr_layer_over and fr_layer_unpremultiply.  The checks, the clipping and
// the tile table are fr_layer_plan.cpp's; this unit stages the table and launches the kernels of fr_layer.hip.
#include "fr_internal.hpp"
#include "fr_layer.hpp"

#include <algorithm>
#include <cstring>
#include <new>

// Room for n tiles in the context's table: pinned staging on the host, which the device reads, and its DevBuf on the
// device, grown on demand.  The earlier table may still be read by a composite in flight, so growing waits for the stream.
static int layer_table_room(fr_ctx *ctx, size_t n)
{
    if (n <= ctx->layer_cap) return FR_OK;
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (ctx->layer_stage) { (void)hipHostFree(ctx->layer_stage); ctx->layer_stage = nullptr; }
    ctx->layer_tab.reset();
    ctx->layer_cap = 0;
    const size_t cap = std::max<size_t>(n + n / 2, 1024);
    hipError_t e = hipHostMalloc(reinterpret_cast<void **>(&ctx->layer_stage), cap * sizeof(fr::LayerTile), hipHostMallocDefault);
    if (e != hipSuccess) { ctx->layer_stage = nullptr; return hip_fail(e, "hipHostMalloc(&ctx->layer_stage, cap)"); }
    ctx->layer_tab.alloc(e, cap * sizeof(fr::LayerTile));
    if (e != hipSuccess) return hip_fail(e, "hipMalloc(&ctx->layer_tab, cap)");
    ctx->layer_cap = cap;
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
    // the table of the call before this one has left the staging (layer_table_kernel reads it in stream order)
    if (ctx->layer_ev) HIP_TRY(hipEventSynchronize(ctx->layer_ev));
    else HIP_TRY(hipEventCreateWithFlags(&ctx->layer_ev, hipEventDisableTiming));
    if (const int rc = layer_table_room(ctx, n)) return rc;
    memcpy(ctx->layer_stage, t.tiles.data(), n * sizeof(fr::LayerTile));
    HIP_TRY(fr::launch_layer_table(ctx->layer_stage, ctx->layer_tab.get(), (uint32_t)n, ctx->stream));
    HIP_TRY(hipEventRecord(ctx->layer_ev, ctx->stream));
    const fr::LayerArgs a{ctx->layer_tab.get(), static_cast<const uint32_t *>(src_dev), static_cast<uint32_t *>(dst_dev), src_stride_px, dst_stride_px};
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

}  // extern "C"

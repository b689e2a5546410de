// fr_api_exact.hip — C ABI (include/fr_raster.h): the exact-integer path (windings of query points and lattices, exact
// coverage) and the glyph debug image built on it.  One-shot calls: every table lives for the call.
#include "fr_internal.hpp"

namespace fr {
void launch_glyph_info(const int16_t *, const uint32_t *, const uint32_t *, uint32_t, int, uint8_t *,
                       uint8_t *, hipStream_t);
void launch_exact_winding(const int16_t *, const uint32_t *, const uint8_t *, const uint8_t *,
                          uint32_t, const int16_t *, uint64_t, uint32_t, int, int, int, int16_t *,
                          hipStream_t);
void launch_exact_cover(const int16_t *, uint32_t, uint32_t, uint32_t, uint8_t *, hipStream_t);
void launch_glyph_debug_color(const int16_t *, uint64_t, uint32_t, uint32_t, uint8_t *, hipStream_t);
}  // namespace fr

struct ExactDev {
    DevBuf<int16_t> pts;
    DevBuf<uint32_t> seg_p0, seg_prev;
    DevBuf<uint8_t> ctype, inc;
    uint32_t n_seg = 0;
    int K = 1;
};

static int exact_setup(fr_ctx *ctx, const int16_t *points_xy, const uint32_t *contour_start,
                       uint32_t n_contours, ExactDev &d, int K = 1)
{
    if (!ctx) return fail(FR_E_INVALID, "ctx is NULL");
    std::vector<uint32_t> seg_p0, seg_prev;
    uint64_t np = 0;
    int rc = fr::flatten_segments(contour_start, n_contours, &np, seg_p0, seg_prev, nullptr);
    if (rc) return rc;
    if (np && !points_xy) return fail(FR_E_INVALID, "points_xy is NULL");
    d.n_seg = (uint32_t)seg_p0.size();
    const size_t ns1 = d.n_seg ? d.n_seg : 1, np1 = np ? np : 1;
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    hipError_t e = hipSuccess;
    d.pts.alloc(e, np1 * 4 + 16);
    d.seg_p0.alloc(e, ns1 * 4);
    d.seg_prev.alloc(e, ns1 * 4);
    d.ctype.alloc(e, ns1);
    d.inc.alloc(e, ns1);
    if (e == hipSuccess && np) e = hipMemcpyAsync(d.pts.get(), points_xy, np * 4, hipMemcpyHostToDevice, st);
    if (e == hipSuccess && d.n_seg) e = hipMemcpyAsync(d.seg_p0.get(), seg_p0.data(), (size_t)d.n_seg * 4, hipMemcpyHostToDevice, st);
    if (e == hipSuccess && d.n_seg) e = hipMemcpyAsync(d.seg_prev.get(), seg_prev.data(), (size_t)d.n_seg * 4, hipMemcpyHostToDevice, st);
    d.K = K;
    if (e == hipSuccess) {
        fr::launch_glyph_info(d.pts.get(), d.seg_p0.get(), d.seg_prev.get(), d.n_seg, K, d.ctype.get(), d.inc.get(), st);
        e = hipGetLastError();
    }
    // (also after a failure: the copies read seg_p0 and seg_prev, which die with this frame)
    const hipError_t e2 = hipStreamSynchronize(st);
    if (e == hipSuccess) e = e2;
    if (e != hipSuccess) return hip_fail(e, "exact set-up");
    return FR_OK;
}

// cover_n > 0: the lattice is (cover_w * cover_n) x (cover_h * cover_n) points and out_host receives
// cover_w x cover_h u8 coverage values instead of the windings
static int exact_run(fr_ctx *ctx, ExactDev &d, const int16_t *query_xy, uint64_t n_query,
                     uint32_t lat_w, int lat_x0, int lat_y0, void *out_host,
                     uint32_t cover_w = 0, uint32_t cover_h = 0, uint32_t cover_n = 0)
{
    if (n_query == 0) return FR_OK;
    if (!out_host) return fail(FR_E_INVALID, "output is NULL");
    if (n_query > 0xffffffffull * 256ull) return fail(FR_E_UNSUPPORTED, "too many query points");
    DevBuf<int16_t> d_q, d_out;
    DevBuf<uint8_t> d_cov;
    hipError_t e = hipSuccess;
    d_out.alloc(e, n_query * 2);
    if (query_xy) d_q.upload(e, query_xy, n_query * 4, ctx->stream);
    if (e == hipSuccess) {
        fr::launch_exact_winding(d.pts.get(), d.seg_p0.get(), d.ctype.get(), d.inc.get(), d.n_seg, d_q.get(), n_query, lat_w, lat_x0, lat_y0, d.K,
                                 d_out.get(), ctx->stream);
        e = hipGetLastError();
    }
    if (cover_n) {
        const size_t npx = (size_t)cover_w * cover_h;
        d_cov.alloc(e, npx ? npx : 1);
        if (e == hipSuccess) {
            fr::launch_exact_cover(d_out.get(), cover_w, cover_h, cover_n, d_cov.get(), ctx->stream);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipMemcpyAsync(out_host, d_cov.get(), npx, hipMemcpyDeviceToHost, ctx->stream);
    } else if (e == hipSuccess) {
        e = hipMemcpyAsync(out_host, d_out.get(), n_query * 2, hipMemcpyDeviceToHost, ctx->stream);
    }
    hipError_t e2 = hipStreamSynchronize(ctx->stream);
    if (e == hipSuccess) e = e2;
    if (e != hipSuccess) return hip_fail(e, "exact winding");
    return FR_OK;
}

extern "C" {

int fr_glyph_info_init(fr_ctx *ctx, const int16_t *points_xy, const uint32_t *contour_start,
                       uint32_t n_contours, uint8_t *curve_type, uint8_t *include_p0)
{
    ExactDev d;
    int rc = exact_setup(ctx, points_xy, contour_start, n_contours, d);
    if (rc) return rc;
    if (d.n_seg) {
        if (!curve_type || !include_p0) return fail(FR_E_INVALID, "output is NULL");
        HIP_TRY(hipMemcpy(curve_type, d.ctype.get(), d.n_seg, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(include_p0, d.inc.get(), d.n_seg, hipMemcpyDeviceToHost));
    }
    return FR_OK;
}

int fr_winding_in_glyph(fr_ctx *ctx, const int16_t *points_xy, const uint32_t *contour_start,
                        uint32_t n_contours, const int16_t *query_xy, uint32_t n_query,
                        int16_t *out_winding)
{
    if (n_query && !query_xy) return fail(FR_E_INVALID, "query_xy is NULL");
    ExactDev d;
    int rc = exact_setup(ctx, points_xy, contour_start, n_contours, d);
    if (rc) return rc;
    return exact_run(ctx, d, query_xy, n_query, 1, 0, 0, out_winding);
}

int fr_winding_lattice(fr_ctx *ctx, const int16_t *points_xy, const uint32_t *contour_start,
                       uint32_t n_contours, const int16_t box[4], int16_t *out_host)
{
    if (!box) return fail(FR_E_INVALID, "box is NULL");
    const int W = (int)box[2] - box[0] + 3, H = (int)box[3] - box[1] + 3;       // Image.zig:183
    if (W < 1 || H < 1) return fail(FR_E_INVALID, "empty box");
    ExactDev d;
    int rc = exact_setup(ctx, points_xy, contour_start, n_contours, d);
    if (rc) return rc;
    return exact_run(ctx, d, nullptr, (uint64_t)W * H, (uint32_t)W, box[0] - 1, box[3] + 1, out_host);
}

int fr_exact_lattice(fr_ctx *ctx, const int16_t *points_xy, const uint32_t *contour_start,
                     uint32_t n_contours, uint32_t K, int32_t x0, int32_t y0, uint32_t w, uint32_t h,
                     int16_t *out_host)
{
    int rc = fr::check_k(K, x0, y0, w, h);
    if (rc) return rc;
    ExactDev d;
    rc = exact_setup(ctx, points_xy, contour_start, n_contours, d, (int)K);
    if (rc) return rc;
    return exact_run(ctx, d, nullptr, (uint64_t)w * h, w, x0, y0, out_host);
}

int fr_exact_coverage(fr_ctx *ctx, const int16_t *points_xy, const uint32_t *contour_start,
                      uint32_t n_contours, uint32_t K, int32_t x0, int32_t y0, uint32_t w_px, uint32_t h_px,
                      uint32_t n, uint8_t *out_host)
{
    if (n < 1 || n > 8) return fail(FR_E_INVALID, "samples per axis must be in [1, 8]");
    int rc = fr::check_k(K, x0, y0, (uint64_t)w_px * n, (uint64_t)h_px * n);
    if (rc) return rc;
    ExactDev d;
    rc = exact_setup(ctx, points_xy, contour_start, n_contours, d, (int)K);
    if (rc) return rc;
    return exact_run(ctx, d, nullptr, (uint64_t)w_px * n * h_px * n, w_px * n, x0, y0, out_host, w_px, h_px, n);
}

int fr_glyph_debug_render(fr_ctx *ctx, const int16_t *points_xy, const uint32_t *contour_start,
                          uint32_t n_contours, const int16_t box[4], uint8_t winding_scale, uint8_t *rgb_host)
{
    if (!box) return fail(FR_E_INVALID, "box is NULL");
    if (!rgb_host) return fail(FR_E_INVALID, "rgb_host is NULL");
    const int W = (int)box[2] - box[0] + 3, H = (int)box[3] - box[1] + 3;       // Image.zig:183
    if (W < 1 || H < 1) return fail(FR_E_INVALID, "empty box");
    ExactDev d;
    int rc = exact_setup(ctx, points_xy, contour_start, n_contours, d);
    if (rc) return rc;
    const uint64_t nq = (uint64_t)W * H;
    DevBuf<int16_t> d_lat;
    DevBuf<uint8_t> d_rgb;
    hipError_t e = hipSuccess;
    d_lat.alloc(e, nq * 2);
    d_rgb.alloc(e, nq * 3);
    if (e == hipSuccess) {
        // the lattice GlyphDebug.render walks (Image.zig:227-236), coloured on the device (setWindingLinear)
        fr::launch_exact_winding(d.pts.get(), d.seg_p0.get(), d.ctype.get(), d.inc.get(), d.n_seg, nullptr, nq, (uint32_t)W, box[0] - 1, box[3] + 1, 1,
                                 d_lat.get(), ctx->stream);
        fr::launch_glyph_debug_color(d_lat.get(), nq, winding_scale, 150u, d_rgb.get(), ctx->stream);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(rgb_host, d_rgb.get(), nq * 3, hipMemcpyDeviceToHost, ctx->stream);
    hipError_t e2 = hipStreamSynchronize(ctx->stream);
    if (e == hipSuccess) e = e2;
    if (e != hipSuccess) return hip_fail(e, "fr_glyph_debug_render");
    // setGlyphPoints (Image.zig:202-218): a few writes in the reference's own order (later points overwrite
    // earlier ones where they coincide), done on the host on the image just copied back
    for (uint32_t c = 0; c < n_contours; ++c) {
        const int16_t *cp = points_xy + 2u * (size_t)contour_start[c];
        const uint32_t curves = (contour_start[c + 1] - contour_start[c]) / 2u;
        for (uint32_t k = 0; k < curves; ++k) {
            for (int which = 0; which < 2; ++which) {
                const int16_t *pt = cp + 2u * (2u * k + (uint32_t)which);
                const int64_t wq = (int64_t)pt[0] - box[0] + 1, hq = (int64_t)box[3] - pt[1] + 1;
                if (wq < 0 || hq < 0 || wq >= W || hq >= H)
                    return fail(FR_E_INVALID, "glyph point outside its box (the reference would write out of bounds)");
                uint8_t *px = rgb_host + 3u * ((size_t)hq * W + (size_t)wq);
                if (which == 0) { px[0] = 255; px[1] = 255; px[2] = 0; }        // on-curve
                else { px[0] = 0; px[1] = 255; px[2] = 255; }                   // control
            }
        }
    }
    return FR_OK;
}

}  // extern "C"

// fr_api_glyph.hip — C ABI (include/fr_raster.h): fr_render_glyph, the reference's call shape (one glyph, one image).
#include "fr_internal.hpp"

#include <cstring>
#include <algorithm>

// One glyph, one image.  No allocation per call: the glyph tables, the job and the output live in the context's device
// arena (grown on demand; glyph_arena, fr_host_rules.hpp), filled by ONE host-to-device copy of a packed staging buffer;
// the render kernel builds the root records in LDS (prepare_kernel runs only for a glyph of more than 128 segments); the
// image comes back with one device-to-host copy.  The job covers the whole image, so the caller's buffer is never
// uploaded.  The launches are those of a plan of this one job (raster_launch) over views of the arena.
extern "C" {

int fr_render_glyph(fr_ctx *ctx, const int16_t *points_xy, const uint32_t *contour_start,
                    uint32_t n_contours, const int16_t box[4], uint16_t units_per_em,
                    uint16_t font_size, int32_t mode, void *out_host)
{
    return fr_render_glyph_ex(ctx, points_xy, contour_start, n_contours, box, units_per_em, font_size, mode, 0u, out_host);
}

int fr_render_glyph_ex(fr_ctx *ctx, const int16_t *points_xy, const uint32_t *contour_start,
                       uint32_t n_contours, const int16_t box[4], uint16_t units_per_em,
                       uint16_t font_size, int32_t mode, uint32_t flags, void *out_host)
{
    if (!ctx) return fail(FR_E_INVALID, "ctx is NULL");
    if (const int frc = fr::check_flags(flags)) return frc;
    int16_t mn[2], mx[2];
    uint16_t w, h;
    float scale;
    int rc = fr_render_glyph_dims(box, units_per_em, font_size, mn, mx, &w, &h, &scale);
    if (rc) return rc;
    fr_raster_params prm{};
    prm.mode = mode; prm.samples_per_axis = 1; prm.sample_phase = FR_SAMPLE_CORNER;
    rc = fr::check_params(&prm);
    if (rc) return rc;
    if (!out_host) return fail(FR_E_INVALID, "out_host is NULL");
    const uint32_t zero_start[1] = {0};
    std::vector<uint32_t> seg_p0, seg_prev;
    uint64_t np = 0;
    rc = fr::flatten_segments(n_contours ? contour_start : zero_start, n_contours, &np, seg_p0, seg_prev, nullptr);
    if (rc) return rc;
    if (np && !points_xy) return fail(FR_E_INVALID, "points_xy is NULL");
    const uint32_t ns = (uint32_t)seg_p0.size();
    if (!fr::scale_in_range(scale)) return fail(FR_E_UNSUPPORTED, "scale outside [2^-20, 2^20]");
    fr_job jb{};
    jb.glyph = 0; jb.min_x = mn[0]; jb.max_y = mx[1]; jb.w = w; jb.h = h; jb.out_x = 0; jb.out_y = 0; jb.scale = scale;
    const size_t img_bytes = (size_t)w * h * (mode == FR_WINDING_I16 ? 2 : 1);
    const fr::GlyphArena o = fr::glyph_arena(np, ns, sizeof(fr::Rec), img_bytes);
    HIP_TRY(hipSetDevice(ctx->device));
    // Option "zero_copy" (off): the kernel reads the tables from, and writes the image to, the pinned staging block
    // itself (host memory mapped into the device's address space).  Measured on STIX 'A' in steady state: 34.9 us per
    // call against 34.7 us with the two small copies — no gain, so the copies stay the default.
    const bool zero_copy = ns <= 128u && mode != FR_SDF_U8 && o.total <= ((size_t)1 << 20) && ctx->zero_copy;
    if (!zero_copy && o.total > ctx->arena_cap) {
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        ctx->arena.reset(); ctx->arena_cap = 0;
        const size_t cap = std::max<size_t>(o.total + o.total / 2, 1u << 20);
        hipError_t ae = hipSuccess;
        ctx->arena.alloc(ae, cap);
        if (ae != hipSuccess) return hip_fail(ae, "hipMalloc(&ctx->arena, cap)");
        ctx->arena_cap = cap;
    }
    const size_t stage_need = zero_copy ? o.total : o.up + img_bytes;
    if (stage_need > ctx->stage_cap) {
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        if (ctx->stage) { (void)hipHostFree(ctx->stage); ctx->stage = nullptr; ctx->stage_cap = 0; }
        const size_t cap = std::max<size_t>(stage_need * 2, 1u << 16);
        HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&ctx->stage), cap, hipHostMallocDefault));
        ctx->stage_cap = cap;
    }
    unsigned char *st = ctx->stage;
    memset(st, 0, o.up);
    if (np) memcpy(st + o.pts, points_xy, np * 4);
    if (ns) memcpy(st + o.p0, seg_p0.data(), (size_t)ns * 4);
    for (uint32_t sgi = 0; sgi < ns; ++sgi) memcpy(st + o.spts + 12u * (size_t)sgi, points_xy + 2u * (size_t)seg_p0[sgi], 12);
    const uint32_t gseg[2] = {0, ns}, jseg[2] = {0, ns}, large0[1] = {0};
    memcpy(st + o.gseg, gseg, 8); memcpy(st + o.job, &jb, sizeof jb); memcpy(st + o.jseg, jseg, 8); memcpy(st + o.large, large0, 4);
    unsigned char *A0 = zero_copy ? st : ctx->arena.get();
    if (!zero_copy) HIP_TRY(hipMemcpyAsync(A0, st, o.up, hipMemcpyHostToDevice, ctx->stream));
    // what the launches read, in the arena: a glyph set of this one glyph (without row cuts) and a plan's tables for its one job
    GlyphView gv{};
    gv.pts = reinterpret_cast<int16_t *>(A0 + o.pts); gv.seg_pts = reinterpret_cast<int16_t *>(A0 + o.spts);
    gv.seg_p0 = reinterpret_cast<uint32_t *>(A0 + o.p0); gv.glyph_seg_start = reinterpret_cast<uint32_t *>(A0 + o.gseg);
    gv.rec_count = reinterpret_cast<uint32_t *>(A0 + o.cnt); gv.recs = reinterpret_cast<fr::Rec *>(A0 + o.recs);
    gv.n_glyphs = 1; gv.max_seg_per_glyph = ns;
    RasterView rv{};
    rv.jobs = reinterpret_cast<fr::Job *>(A0 + o.job); rv.job_seg = reinterpret_cast<uint32_t *>(A0 + o.jseg);
    rv.large = reinterpret_cast<uint32_t *>(A0 + o.large);
    fr::RasterPlan rp;
    {
        // the same rules as fr_plan_create, for this one job: the image takes win1_kernel (64- / 128- / 256-pixel strips by its
        // own width) unless the glyph is too large for it (single_glyph_in: what differs from a plan's job)
        std::vector<std::pair<int32_t, int32_t>> ev;
        const uint32_t root = fr::glyph_root_bound(points_xy, seg_p0.data(), 0, ns), ray = fr::glyph_ray_bound(points_xy, seg_p0.data(), 0, ns, ev);
        const fr::RasterPlanIn in = fr::single_glyph_in(&jb, gseg, &root, &ray, prm);
        uint8_t cls1;
        uint32_t order1, jseg1[2], large1, jbits1;
        fr_job sorted1;
        const fr::RasterTables t1 = {&cls1, &order1, &sorted1, jseg1, &large1, &jbits1};
        fr::raster_plan_build(in, raster_opts(ctx), t1, rp);
        fr::raster_plan_tables(in, t1, rp);
    }
    int lrc = FR_OK;
    if (mode == FR_SDF_U8 || rp.n_large) {
        // the stand-alone records (float brackets): the staged path of a large glyph and the SDF's stand-alone users
        hipError_t e = hipMemsetAsync(gv.rec_count, 0, 8, ctx->stream);
        if (e != hipSuccess) lrc = fail(FR_E_HIP, "hipMemsetAsync: %s", hipGetErrorString(e));
    }
    if (lrc == FR_OK) lrc = raster_launch(ctx, gv, rv, rp, prm, flags, A0 + o.out, w);
    hipError_t e = hipSuccess;
    if (lrc == FR_OK && !zero_copy) e = hipMemcpyAsync(st + o.up, A0 + o.out, img_bytes, hipMemcpyDeviceToHost, ctx->stream);
    hipError_t e2 = hipStreamSynchronize(ctx->stream);
    if (lrc == FR_OK && e == hipSuccess && e2 == hipSuccess) memcpy(out_host, zero_copy ? st + o.out : st + o.up, img_bytes);
    if (lrc) return lrc;
    if (e == hipSuccess) e = e2;
    if (e != hipSuccess) return fail(FR_E_HIP, "fr_render_glyph: %s", hipGetErrorString(e));
    return FR_OK;
}

}  // extern "C"

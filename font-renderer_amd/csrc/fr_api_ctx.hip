// fr_api_ctx.hip — C ABI (include/fr_raster.h): the error text, contexts and their options, glyph sets.
#include "fr_internal.hpp"

#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <algorithm>
#include <new>

namespace fr {
// fill = 1: the FR_FILL_CONSISTENT instances (fr_records.hpp)
void launch_prepare(const int16_t *, const uint32_t *, const uint32_t *, const uint32_t *, uint32_t, Rec *,
                    uint32_t *, hipStream_t, int fill = 0);
void launch_cuts(const int16_t *, uint32_t, float4 *, hipStream_t);
void launch_cands(const int16_t *, const uint32_t *, const float4 *, uint32_t, uint4 *, hipStream_t);
void launch_selftest_cand_records(const uint32_t *, const int16_t *, const uint4 *, uint32_t, unsigned long long *, uint32_t *, hipStream_t);
void launch_selftest_row_cuts(const Job *, uint32_t, uint32_t, const uint32_t *, const int16_t *, const float4 *, int, int,
                              unsigned long long *, hipStream_t);
uint32_t cov4_max_segments();
}  // namespace fr

static_assert(sizeof(fr_job) == sizeof(fr::Job), "fr_job layout");
static_assert(sizeof(fr_job) == 32, "fr_job is 32 bytes");

// --------------------------------------------------------------------------
static thread_local char g_err[512] = "";

namespace fr {
int set_error(int code, const char *fmt, ...)          // every unit of the library reports through it (`fail`)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
    return code;
}
}  // namespace fr

fr_glyphset::~fr_glyphset()
{
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
}

extern "C" {

int fr_abi_version(void) { return FR_ABI_VERSION; }
const char *fr_last_error(void) { return g_err; }
#ifndef FR_BUILD_ID
#error "FR_BUILD_ID comes from the Makefile (a hash of the sources)"
#endif
const char *fr_build_id(void) { return FR_BUILD_ID; }

int fr_ctx_create(int device, void *hip_stream, fr_ctx **out)
{
    if (!out) return fail(FR_E_INVALID, "fr_ctx_create: out is NULL");
    *out = nullptr;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0)
        return fail(FR_E_HIP, "fr_ctx_create: no HIP device (%s); this library has no CPU path",
                    e != hipSuccess ? hipGetErrorString(e) : "count = 0");
    if (device < 0 || device >= n) return fail(FR_E_INVALID, "fr_ctx_create: device %d of %d", device, n);
    if (fr::cov4_max_segments() != fr::COV4_MAX_SEGMENTS)          // (fast_class, plain host code, against the kernel unit's own figure)
        return fail(FR_E_UNSUPPORTED, "fr_ctx_create: fast_class takes %u segments, cov4_kernel %u", fr::COV4_MAX_SEGMENTS, fr::cov4_max_segments());
    HIP_TRY(hipSetDevice(device));
    fr_ctx *c = new (std::nothrow) fr_ctx;
    if (!c) return fail(FR_E_NOMEM, "fr_ctx_create: host allocation");
    c->device = device;
    if (hip_stream) {
        c->stream = static_cast<hipStream_t>(hip_stream);
    } else {
        e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
        if (e != hipSuccess) { delete c; return fail(FR_E_HIP, "hipStreamCreate: %s", hipGetErrorString(e)); }
        c->owns_stream = true;
    }
    *out = c;
    return FR_OK;
}

void fr_ctx_destroy(fr_ctx *ctx)
{
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    ctx->arena.reset();
    if (ctx->stage) (void)hipHostFree(ctx->stage);
    ctx->layer_tab.reset();
    if (ctx->layer_stage) (void)hipHostFree(ctx->layer_stage);
    if (ctx->layer_ev) (void)hipEventDestroy(ctx->layer_ev);
    if (ctx->aux) { (void)hipStreamSynchronize(ctx->aux); (void)hipStreamDestroy(ctx->aux); }
    if (ctx->ev_fork) (void)hipEventDestroy(ctx->ev_fork);
    if (ctx->ev_join) (void)hipEventDestroy(ctx->ev_join);
    if (ctx->owns_stream) (void)hipStreamDestroy(ctx->stream);
    delete ctx;
}

int fr_ctx_sync(fr_ctx *ctx)
{
    if (!ctx) return fail(FR_E_INVALID, "fr_ctx_sync: ctx is NULL");
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return FR_OK;
}

// The option keys.  A switch (lo == hi == 0) takes any value as on / off; a range refuses what lies outside [lo, hi] or is
// no multiple of `step` with `refusal`.  `launch`: the option feeds the launches of a plan's render, so a successful set
// moves opt_epoch and captured graphs are captured again.  ("graph" and "zero_copy" change no launch of a plan; a
// refused or unknown option changes nothing at all.)
int fr_ctx_set_option(fr_ctx *ctx, const char *key, int64_t value)
{
    if (!ctx || !key) return fail(FR_E_INVALID, "fr_ctx_set_option: NULL argument");
    static const struct {
        const char *key;
        uint32_t fr_ctx::*field;
        bool launch;
        int64_t lo, hi, step;
        const char *refusal;
    } OPTS[] = {
        {"graph", &fr_ctx::graph, false, 0, 0, 1, nullptr},
        {"kmax", &fr_ctx::kmax, true, 1, 128, 1, "kmax must be in [1,128]"},
        {"strip_px", &fr_ctx::strip_px, true, 16, 256, 16, "strip_px must be a multiple of 16 in [16,256]"},
        {"fuse_prepare", &fr_ctx::fuse_prepare, true, 0, 0, 1, nullptr},
        {"lds_pad", &fr_ctx::lds_pad, true, 0, 0xffffffffll, 1, nullptr},           // (taken modulo 2^32)
        {"cov4", &fr_ctx::cov4, true, 0, 0, 1, nullptr},
        {"row_cuts", &fr_ctx::row_cuts, true, 0, 0, 1, nullptr},
        {"cand_records", &fr_ctx::cand_records, true, 0, 0, 1, nullptr},
        {"sdf_cull", &fr_ctx::sdf_cull, true, 0, 0, 1, nullptr},
        {"overlap", &fr_ctx::overlap, true, 0, 2, 1, "overlap must be 0 (never), 1 (plans of >= 32 Mpixel) or 2 (always)"},
        {"zero_copy", &fr_ctx::zero_copy, false, 0, 0, 1, nullptr},
        {"min_wgs", &fr_ctx::min_wgs, true, 1, 1 << 24, 1, "min_wgs out of range"},
    };
    for (const auto &o : OPTS) {
        if (strcmp(key, o.key)) continue;
        if (o.hi == 0) {
            ctx->*o.field = value ? 1u : 0u;
        } else {
            if (o.refusal && (value < o.lo || value > o.hi || (value % o.step))) return fail(FR_E_INVALID, "%s", o.refusal);
            ctx->*o.field = (uint32_t)value;
        }
        if (o.launch) ++ctx->opt_epoch;
        return FR_OK;
    }
    return fail(FR_E_INVALID, "fr_ctx_set_option: unknown key '%s'", key);
}

// ---- glyph tables (flatten_segments and the two glyph bounds: fr_raster_plan.cpp) ---------------------------------------
void fr_glyphset_destroy(fr_glyphset *gs) { delete gs; }

int fr_glyphset_prepare(fr_glyphset *gs)
{
    if (!gs) return fail(FR_E_INVALID, "fr_glyphset_prepare: NULL");
    HIP_TRY(hipSetDevice(gs->ctx->device));
    fr::launch_prepare(gs->pts.get(), gs->seg_p0.get(), gs->glyph_seg_start.get(), nullptr, gs->n_glyphs, gs->recs.get(),
                       gs->rec_count.get(), gs->ctx->stream);
    HIP_TRY(hipGetLastError());
    return FR_OK;
}

int fr_glyphset_create(fr_ctx *ctx, const int16_t *points_xy, const uint32_t *contour_start,
                       uint32_t n_contours, const uint32_t *glyph_start, uint32_t n_glyphs,
                       fr_glyphset **out)
{
    if (!ctx || !out) return fail(FR_E_INVALID, "fr_glyphset_create: NULL argument");
    *out = nullptr;
    if (n_glyphs && !glyph_start) return fail(FR_E_INVALID, "glyph_start is NULL");
    if (n_glyphs && (glyph_start[0] != 0 || glyph_start[n_glyphs] != n_contours))
        return fail(FR_E_INVALID, "glyph_start must run from 0 to n_contours");
    std::vector<uint32_t> seg_p0, seg_prev, cseg;
    uint64_t np = 0;
    int rc = fr::flatten_segments(contour_start, n_contours, &np, seg_p0, seg_prev, &cseg);
    if (rc) return rc;
    if (np && !points_xy) return fail(FR_E_INVALID, "points_xy is NULL");
    if (seg_p0.size() > 0x7fffffffull) return fail(FR_E_UNSUPPORTED, "too many segments");
    std::vector<uint32_t> gseg(n_glyphs + 1, 0u);
    for (uint32_t g = 0; g < n_glyphs; ++g) {
        if (glyph_start[g + 1] < glyph_start[g] || glyph_start[g + 1] > n_contours)
            return fail(FR_E_INVALID, "glyph_start not monotone at %u", g);
        gseg[g + 1] = cseg[glyph_start[g + 1]];
    }
    uint32_t max_seg = 0;
    for (uint32_t g = 0; g < n_glyphs; ++g) max_seg = std::max(max_seg, gseg[g + 1] - gseg[g]);
    std::vector<uint32_t> root_bound(n_glyphs, 0u), ray_bound(n_glyphs, 0u);
    {
        std::vector<std::pair<int32_t, int32_t>> ev;
        for (uint32_t g = 0; g < n_glyphs; ++g) {
            root_bound[g] = fr::glyph_root_bound(points_xy, seg_p0.data(), gseg[g], gseg[g + 1]);
            ray_bound[g] = fr::glyph_ray_bound(points_xy, seg_p0.data(), gseg[g], gseg[g + 1], ev);
        }
    }
    std::vector<int16_t> seg_pts(seg_p0.size() * 6);
    for (size_t sgi = 0; sgi < seg_p0.size(); ++sgi) memcpy(&seg_pts[6 * sgi], points_xy + 2u * (size_t)seg_p0[sgi], 12);
    HIP_TRY(hipSetDevice(ctx->device));
    // declared behind the host vectors the copies read: whatever fails below, ~fr_glyphset waits for the stream first
    std::unique_ptr<fr_glyphset> gs(new (std::nothrow) fr_glyphset);
    if (!gs) return fail(FR_E_NOMEM, "fr_glyphset_create: host allocation");
    gs->ctx = ctx; gs->n_glyphs = n_glyphs; gs->n_contours = n_contours;
    gs->n_seg = (uint32_t)seg_p0.size(); gs->n_points = np; gs->max_seg_per_glyph = max_seg;
    const size_t nseg1 = gs->n_seg ? gs->n_seg : 1, np1 = np ? np : 1, ng1 = (size_t)n_glyphs + 1;
    hipStream_t st = ctx->stream;
    hipError_t e = hipSuccess;
    gs->pts.alloc(e, np1 * 2 * sizeof(int16_t) + 16);
    gs->seg_pts.alloc(e, nseg1 * 12 + 16);
    gs->seg_p0.alloc(e, nseg1 * 4);
    gs->seg_prev.alloc(e, nseg1 * 4);
    gs->glyph_seg_start.alloc(e, ng1 * 4);
    gs->rec_count.alloc(e, ng1 * 4);
    gs->recs.alloc(e, 2 * nseg1 * sizeof(fr::Rec));
    gs->seg_cut.alloc(e, nseg1 * sizeof(float4));
    gs->seg_cand.alloc(e, nseg1 * 6 * sizeof(uint4));
    if (e == hipSuccess && np) e = hipMemcpyAsync(gs->pts.get(), points_xy, np * 2 * sizeof(int16_t), hipMemcpyHostToDevice, st);
    if (e == hipSuccess && gs->n_seg) e = hipMemcpyAsync(gs->seg_pts.get(), seg_pts.data(), (size_t)gs->n_seg * 12, hipMemcpyHostToDevice, st);
    if (e == hipSuccess && gs->n_seg) e = hipMemcpyAsync(gs->seg_p0.get(), seg_p0.data(), (size_t)gs->n_seg * 4, hipMemcpyHostToDevice, st);
    if (e == hipSuccess && gs->n_seg) e = hipMemcpyAsync(gs->seg_prev.get(), seg_prev.data(), (size_t)gs->n_seg * 4, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(gs->glyph_seg_start.get(), gseg.data(), ng1 * 4, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemsetAsync(gs->rec_count.get(), 0, ng1 * 4, st);
    if (e == hipSuccess) {
        fr::launch_prepare(gs->pts.get(), gs->seg_p0.get(), gs->glyph_seg_start.get(), nullptr, n_glyphs, gs->recs.get(),
                           gs->rec_count.get(), st);
        e = hipGetLastError();
    }
    if (e == hipSuccess) {
        fr::launch_cuts(gs->seg_pts.get(), gs->n_seg, gs->seg_cut.get(), st);     // the row cuts: once, they hold for every cell and scale
        e = hipGetLastError();
    }
    if (e == hipSuccess) {
        // the candidate table, from the cuts: once, it holds for every cell and scale
        fr::launch_cands(gs->seg_pts.get(), gs->glyph_seg_start.get(), gs->seg_cut.get(), n_glyphs, gs->seg_cand.get(), st);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(st);   // host vectors above die with this frame
    if (e != hipSuccess) return hip_fail(e, "fr_glyphset_create");
    gs->h_glyph_seg_start = std::move(gseg);
    gs->h_root_bound = std::move(root_bound);
    gs->h_ray_bound = std::move(ray_bound);
    *out = gs.release();
    return FR_OK;
}

int fr_glyphset_stats(const fr_glyphset *gs, uint64_t *n_segments, uint64_t *n_records)
{
    if (!gs) return fail(FR_E_INVALID, "fr_glyphset_stats: NULL");
    HIP_TRY(hipSetDevice(gs->ctx->device));
    if (n_segments) *n_segments = gs->n_seg;
    if (n_records) {
        std::vector<uint32_t> cnt(gs->n_glyphs + 1);
        HIP_TRY(hipStreamSynchronize(gs->ctx->stream));
        HIP_TRY(hipMemcpy(cnt.data(), gs->rec_count.get(), ((size_t)gs->n_glyphs) * 4, hipMemcpyDeviceToHost));
        uint64_t t = 0;
        for (uint32_t g = 0; g < gs->n_glyphs; ++g) t += cnt[g];
        *n_records = t;
    }
    return FR_OK;
}

int fr_glyphset_set_boxes(fr_glyphset *gs, const int16_t *boxes)
{
    if (!gs || (gs->n_glyphs && !boxes)) return fail(FR_E_INVALID, "fr_glyphset_set_boxes: NULL argument");
    for (uint32_t g = 0; g < gs->n_glyphs; ++g)
        if (boxes[4 * (size_t)g] > boxes[4 * (size_t)g + 2] || boxes[4 * (size_t)g + 1] > boxes[4 * (size_t)g + 3])
            return fail(FR_E_INVALID, "glyph %u: box min above max", g);
    gs->h_box.assign(boxes, boxes + 4 * (size_t)gs->n_glyphs);
    return FR_OK;
}

int fr_selftest_row_cuts(fr_glyphset *gs, const fr_job *jobs, uint32_t n_jobs, int samples_per_axis, int phase,
                         uint64_t *pairs, uint64_t *mismatches, uint32_t *first_bad)
{
    if (!gs || !pairs || !mismatches) return fail(FR_E_INVALID, "fr_selftest_row_cuts: NULL argument");
    if (n_jobs && !jobs) return fail(FR_E_INVALID, "jobs is NULL");
    const int n = samples_per_axis;
    if (n != 1 && n != 2 && n != 4) return fail(FR_E_UNSUPPORTED, "samples_per_axis %d not in {1,2,4}", n);
    if (phase != FR_SAMPLE_CORNER && phase != FR_SAMPLE_CENTER) return fail(FR_E_INVALID, "unknown sample_phase %d", phase);
    if (!gs->seg_cut.get()) return fail(FR_E_INVALID, "fr_selftest_row_cuts: the glyph set has no row cuts");
    uint32_t max_rows = 0;
    for (uint32_t j = 0; j < n_jobs; ++j) {
        if (const int jrc = fr::check_job(gs->n_glyphs, jobs[j], j)) return jrc;
        max_rows = std::max(max_rows, jobs[j].h * (uint32_t)n);
    }
    *pairs = 0; *mismatches = 0;
    if (first_bad) first_bad[0] = first_bad[1] = first_bad[2] = 0u;
    if (n_jobs == 0 || max_rows == 0) return FR_OK;
    HIP_TRY(hipSetDevice(gs->ctx->device));
    hipStream_t st = gs->ctx->stream;
    DevBuf<fr::Job> d_jobs;
    DevBuf<unsigned long long> d_res;
    unsigned long long res[3] = {0ull, 0ull, ~0ull};
    hipError_t e = hipSuccess;
    d_jobs.alloc(e, (size_t)n_jobs * sizeof(fr::Job));
    d_res.alloc(e, sizeof res);
    if (e == hipSuccess) e = hipMemcpyAsync(d_jobs.get(), jobs, (size_t)n_jobs * sizeof(fr::Job), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(d_res.get(), res, sizeof res, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) {
        fr::launch_selftest_row_cuts(d_jobs.get(), n_jobs, max_rows, gs->glyph_seg_start.get(), gs->seg_pts.get(), gs->seg_cut.get(), n,
                                     phase == FR_SAMPLE_CENTER ? 1 : 0, d_res.get(), st);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(res, d_res.get(), sizeof res, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    else (void)hipStreamSynchronize(st);                  // (the copies above read `jobs` and `res`)
    if (e != hipSuccess) return hip_fail(e, "fr_selftest_row_cuts");
    *pairs = res[0];
    *mismatches = res[1];
    if (first_bad && res[1]) {
        first_bad[0] = (uint32_t)(res[2] >> 40); first_bad[1] = (uint32_t)((res[2] >> 20) & 0xfffffu); first_bad[2] = (uint32_t)(res[2] & 0xfffffu);
    }
    return FR_OK;
}

int fr_selftest_cand_records(fr_glyphset *gs, uint64_t *live, uint64_t *mismatches, uint32_t *first_bad, uint32_t *glyph_live)
{
    if (!gs || !live || !mismatches) return fail(FR_E_INVALID, "fr_selftest_cand_records: NULL argument");
    if (!gs->seg_cand.get()) return fail(FR_E_INVALID, "fr_selftest_cand_records: the glyph set has no candidate table");
    *live = 0; *mismatches = 0;
    if (first_bad) first_bad[0] = first_bad[1] = 0u;
    if (gs->n_glyphs == 0) return FR_OK;
    HIP_TRY(hipSetDevice(gs->ctx->device));
    hipStream_t st = gs->ctx->stream;
    DevBuf<unsigned long long> d_res;
    DevBuf<uint32_t> d_live;
    unsigned long long res[3] = {0ull, 0ull, ~0ull};
    std::vector<uint32_t> h_live(gs->n_glyphs, 0u);
    hipError_t e = hipSuccess;
    d_res.alloc(e, sizeof res);
    d_live.alloc(e, (size_t)gs->n_glyphs * 4);
    if (e == hipSuccess) e = hipMemcpyAsync(d_res.get(), res, sizeof res, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) {
        fr::launch_selftest_cand_records(gs->glyph_seg_start.get(), gs->seg_pts.get(), gs->seg_cand.get(), gs->n_glyphs, d_res.get(),
                                         d_live.get(), st);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(res, d_res.get(), sizeof res, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(h_live.data(), d_live.get(), (size_t)gs->n_glyphs * 4, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    else (void)hipStreamSynchronize(st);                  // (the copies above read and write `res` and `h_live`)
    if (e != hipSuccess) return hip_fail(e, "fr_selftest_cand_records");
    *live = res[0];
    *mismatches = res[1];
    if (first_bad && res[1]) { first_bad[0] = (uint32_t)(res[2] >> 32); first_bad[1] = (uint32_t)res[2]; }
    if (glyph_live) memcpy(glyph_live, h_live.data(), (size_t)gs->n_glyphs * 4);
    return FR_OK;
}

}  // extern "C"

// fr_api.hip — host side of libfr_raster.so: the C ABI of include/fr_raster.h.
//
// Owns device memory (glyph tables, root records, job tables), validates what the
// caller hands over, and launches the kernels of fr_prepare.hip / fr_render.hip /
// fr_exact.hip on the context's HIP stream.  No CPU rasterization path exists here:
// without a usable gfx950 device every compute entry point returns FR_E_HIP.
#include "../../include/fr_raster.h"
#include "fr_device.hpp"
#include "fr_srgb.hpp"
#include "fr_text.hpp"
#include "fr_raster_plan.hpp"
#include "fr_text_plan.hpp"

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <new>
#include <algorithm>
#include <dlfcn.h>
#include <type_traits>
#include <vector>

namespace fr {
// fill = 1: the FR_FILL_CONSISTENT instances (fr_records.hpp)
void launch_prepare(const int16_t *, const uint32_t *, const uint32_t *, const uint32_t *, uint32_t, Rec *,
                    uint32_t *, hipStream_t, int fill = 0);
void launch_cuts(const int16_t *, uint32_t, float4 *, hipStream_t);
void launch_selftest_row_cuts(const Job *, uint32_t, uint32_t, const uint32_t *, const int16_t *, const float4 *, int, int,
                              unsigned long long *, hipStream_t);
hipError_t launch_render(const RenderArgs &, const RasterLaunch &, hipStream_t);
uint32_t render_wg_waves();
hipError_t launch_cov4(const RenderArgs &, const RasterLaunch &, hipStream_t);
hipError_t launch_win1(const RenderArgs &, const RasterLaunch &, hipStream_t);
uint32_t cov4_wg_waves();
uint32_t cov4_max_segments();
hipError_t launch_sdf(const RenderArgs &, uint32_t, uint32_t, uint32_t max_seg, int cull, hipStream_t);
void launch_glyph_info(const int16_t *, const uint32_t *, const uint32_t *, uint32_t, int, uint8_t *,
                       uint8_t *, hipStream_t);
void launch_exact_winding(const int16_t *, const uint32_t *, const uint8_t *, const uint8_t *,
                          uint32_t, const int16_t *, uint64_t, uint32_t, int, int, int, int16_t *,
                          hipStream_t);
void launch_exact_cover(const int16_t *, uint32_t, uint32_t, uint32_t, uint8_t *, hipStream_t);
void launch_glyph_debug_color(const int16_t *, uint64_t, uint32_t, uint32_t, uint8_t *, hipStream_t);
}  // namespace fr

static_assert(sizeof(fr_job) == sizeof(fr::Job), "fr_job layout");
static_assert(sizeof(fr_job) == 32, "fr_job is 32 bytes");

// --------------------------------------------------------------------------
static thread_local char g_err[512] = "";

static int fail(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
    return code;
}
namespace fr {
int set_error(int code, const char *fmt, ...)          // for the other translation units (fr_font.cpp)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
    return code;
}
}  // namespace fr
#define HIP_TRY(expr)                                                                        \
    do {                                                                                     \
        hipError_t e_ = (expr);                                                              \
        if (e_ != hipSuccess)                                                                \
            return fail(e_ == hipErrorOutOfMemory ? FR_E_NOMEM : FR_E_HIP, "%s: %s", #expr,  \
                        hipGetErrorString(e_));                                              \
    } while (0)

struct fr_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    bool owns_stream = false;
    uint32_t kmax = 32;          // crossings kept per sample row (register array: 8, 16 or 32) before the direct-sum fallback
    uint32_t strip_px = 256;     // column strip width, pixels (multiple of 16, <= 256)
    uint32_t fuse_prepare = 1;   // build root records inside the render kernel when every glyph has <= 128 segments
    uint32_t lds_pad = 0;        // experiment knob: extra dynamic LDS bytes per workgroup (occupancy studies)
    uint32_t min_wgs = 2048;     // split a cell's bands over workgroups below this many workgroups
    uint32_t cov4 = 1;           // jobs take the fast kernels (cov4_kernel / win1_kernel) where they fit (fast_class); 0: all general
    uint32_t row_cuts = 1;       // the fast kernels' set-up reads a row's class off the glyph set's row cuts; 0: evaluates the reference's acceptance
    uint32_t zero_copy = 0;      // fr_render_glyph: render small glyphs from / into pinned host memory directly (measured: no faster than two small copies; off)
    uint32_t sdf_cull = 1;       // FR_SDF_U8: drop segments that cannot change a tile / a pixel (exact; 0 = look at all, for tests)
    uint32_t overlap = 1;        // a plan's smaller launches run beside its largest one on a second stream: 0 never, 1 plans of >= 32 Mpixel, 2 always
    uint32_t graph = 0;          // 1: a plan's launches are captured into a hipGraph at its first render to a destination and replayed afterwards
    uint32_t opt_epoch = 0;      // bumped by every fr_ctx_set_option: a captured graph is only replayed under the options it was captured with
    hipStream_t aux = nullptr;   // that second stream and the fork / join events, created on first use
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    // scratch of the single-glyph entry point (fr_render_glyph): one device arena and one host staging
    // buffer, grown on demand and reused across calls
    unsigned char *arena = nullptr;
    size_t arena_cap = 0;
    unsigned char *stage = nullptr;     // pinned host memory: [upload block | image coming back]
    size_t stage_cap = 0;
};

struct fr_glyphset {
    fr_ctx *ctx = nullptr;
    uint32_t n_glyphs = 0, n_contours = 0, n_seg = 0, max_seg_per_glyph = 0;
    uint64_t n_points = 0;
    int16_t *d_pts = nullptr, *d_seg_pts = nullptr;
    uint32_t *d_seg_p0 = nullptr, *d_seg_prev = nullptr, *d_glyph_seg_start = nullptr, *d_rec_count = nullptr;
    fr::Rec *d_recs = nullptr;
    float4 *d_seg_cut = nullptr;                // row cuts, one float4 per segment (fr_records.hpp): 16 B per segment.  Null in
                                                // the glyph set fr_render_glyph dresses its arena as
    std::vector<uint32_t> h_glyph_seg_start;   // host copy: plans attach each job's segment range to it
    std::vector<uint32_t> h_root_bound;         // per glyph: candidate roots the vertex rule cannot discard (>= live records)
    std::vector<uint32_t> h_ray_bound;          // per glyph: estimated maximum of the crossings of one horizontal ray
    std::vector<int16_t> h_box;                 // fr_glyphset_set_boxes: Glyph.box per glyph (x_min, y_min, x_max, y_max); empty until set
};

struct fr_plan {
    fr_ctx *ctx = nullptr;
    const fr_glyphset *gs = nullptr;
    fr::Job *d_jobs = nullptr;
    uint32_t *d_job_seg = nullptr;     // [n_jobs][2]: first segment and segment count of the job's glyph
    uint32_t *d_bits = nullptr;        // FR_SDF_U8: the sign bit planes of the fast kernels' jobs (one bit per pixel: fr_win1.hip)
    uint32_t *d_job_bits = nullptr;    // and each job's first word in them (0xffffffff: a general-kernel job)
    uint32_t *d_large = nullptr;       // distinct glyphs of more than 128 segments among the general jobs (rp.n_large): their records
                                       // are rebuilt by prepare_kernel before every render (the others: inside the render kernel)
    // the job classes, the parts and the launch geometry (fr_raster_plan.hpp); d_jobs / d_job_seg hold the jobs in its order.
    // A text plan uses its pixels, need_cols and need_rows only
    fr::RasterPlan rp;
    fr_raster_params params{};
    uint32_t flags = 0;                // fr_plan_create_ex's flags (FR_FILL_CONSISTENT)
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    // option "graph": the launches of one render as an instantiated hipGraph, and what it was captured for
    hipGraphExec_t gexec = nullptr;
    void *g_out = nullptr;
    size_t g_stride = 0, g_rows = 0;
    uint32_t g_epoch = 0;
    // a text plan (fr_text_plan_create): what its launches depend on (fr_text_plan.hpp), its tables (fr_text.hpp) and the
    // distinct glyphs whose records prepare_kernel rebuilds into plan-owned memory before every render
    bool text = false;
    fr::TextPlan tp;
    fr::TextTile *d_tiles = nullptr;
    fr::TextRun *d_runs = nullptr;
    void *d_insts = nullptr;           // TextInst, TextInstEx or TextInstAffine (tp.form); tp.cached: TextCachedInst
    uint32_t *d_tlist = nullptr, *d_tglyphs = nullptr, *d_trec_count = nullptr;
    fr::Rec *d_trecs = nullptr;
    // tp.cached: a render fills the mask store from the cells' tiles between the prepare kernel and the composite
    // (fr_text_cached.hip)
    fr::TextMaskCell *d_mcells = nullptr;
    fr::TextMaskTile *d_mtiles = nullptr;
    uint16_t *d_masks = nullptr;
};

template <class T> static void dfree(T *&p) { if (p) { (void)hipFree(p); p = nullptr; } }

static fr::RasterOpts raster_opts(const fr_ctx *ctx)
{
    return fr::RasterOpts{ctx->strip_px, ctx->cov4, ctx->fuse_prepare, ctx->min_wgs, ctx->overlap, fr::render_wg_waves(), fr::cov4_wg_waves(), ctx->kmax};
}

// what every launch of a raster plan's render shares; launch_entry adds the entry's jobs and geometry
static fr::RenderArgs render_args(const fr_plan *plan, void *out_dev, size_t out_stride)
{
    fr::RenderArgs a{};
    a.glyph_seg_start = plan->gs->d_glyph_seg_start;
    a.glyph_rec_count = plan->gs->d_rec_count;
    a.recs = plan->gs->d_recs;
    a.pts = plan->gs->d_pts;
    a.seg_p0 = plan->gs->d_seg_p0;
    a.seg_pts = plan->gs->d_seg_pts;
    a.seg_cut = plan->ctx->row_cuts ? plan->gs->d_seg_cut : nullptr;
    // fused: the render kernel builds the records of every glyph of <= 128 segments (<= 256 candidate roots)
    // in LDS itself — decided per job inside the kernel; larger glyphs are staged from HBM
    a.fused = plan->ctx->fuse_prepare ? 1u : 0u;
    a.out = out_dev;
    a.out_stride = out_stride;
    a.kmax = plan->ctx->kmax;
    a.phase_center = plan->params.sample_phase == FR_SAMPLE_CENTER ? 1 : 0;
    a.lds_pad = plan->ctx->lds_pad;
    return a;
}

// one entry of a plan's launch list (fr_raster_plan.hpp) on stream `st`
static hipError_t launch_entry(const fr_plan *plan, fr::RenderArgs a, const fr::RasterLaunch &e, hipStream_t st)
{
    const fr_glyphset *gs = plan->gs;
    a.jobs = plan->d_jobs + e.first;
    a.job_seg = plan->d_job_seg + 2u * (size_t)e.first;
    a.n_jobs = e.cnt; a.bands = e.bands; a.strips = e.strips; a.strip_w = e.strip_w; a.uniform = e.uniform ? 1u : 0u;
    a.bands_per_wg = e.bands_per_wg; a.band_groups = e.band_groups;
    switch (e.family) {
    case fr::RL_PREPARE:
        fr::launch_prepare(gs->d_pts, gs->d_seg_p0, gs->d_glyph_seg_start, e.cnt ? plan->d_large : nullptr,
                           e.cnt ? e.cnt : gs->n_glyphs, gs->d_recs, gs->d_rec_count, st, e.mode);
        return hipSuccess;
    case fr::RL_RENDER: return fr::launch_render(a, e, st);
    case fr::RL_COV4: return fr::launch_cov4(a, e, st);
    case fr::RL_WIN1:
        if (e.mode == 3) { a.out = plan->d_bits; a.job_bits = plan->d_job_bits + e.first; }     // the sign pass writes the bit planes
        return fr::launch_win1(a, e, st);
    default:                                                                                    // RL_SDF
        a.bits = plan->d_bits; a.job_bits = plan->d_job_bits;
        return fr::launch_sdf(a, plan->rp.max_w, plan->rp.max_h, gs->max_seg_per_glyph, (int)plan->ctx->sdf_cull, st);
    }
}

// the TextTables part of what a text kernel reads, over the plan's instance table as the record type of ARGS
// (fr::TextArgs, fr::TextPlaceArgs, fr::TextAffineArgs or fr::TextCachedArgs, whose kernels do not read the records)
template <class ARGS>
static ARGS text_args(const fr_plan *plan, void *out_dev, size_t out_stride)
{
    ARGS a{};
    a.tiles = plan->d_tiles; a.runs = plan->d_runs; a.list = plan->d_tlist;
    a.insts = static_cast<decltype(a.insts)>(plan->d_insts);
    a.recs = plan->d_trecs; a.rec_count = plan->d_trec_count;
    a.out = static_cast<uint8_t *>(out_dev);
    a.out_stride = out_stride;
    a.phase_center = plan->params.sample_phase == FR_SAMPLE_CENTER ? 1 : 0;
    return a;
}

// one entry of a text plan's launch list (fr_text_plan.hpp) on the context's stream
static hipError_t text_launch_entry(const fr_plan *plan, const fr::TextLaunch &e, void *out_dev, size_t out_stride)
{
    const fr_glyphset *gs = plan->gs;
    hipStream_t st = plan->ctx->stream;
    switch (e.family) {
    case fr::TL_PREPARE:
        fr::launch_prepare(gs->d_pts, gs->d_seg_p0, gs->d_glyph_seg_start, plan->d_tglyphs, e.grid, plan->d_trecs, plan->d_trec_count, st, e.fill);
        return hipGetLastError();
    case fr::TL_MASK: {
        fr::TextMaskArgs a;
        a.tiles = plan->d_mtiles; a.cells = plan->d_mcells;
        a.recs = plan->d_trecs; a.rec_count = plan->d_trec_count;
        a.masks = plan->d_masks;
        a.phase_center = plan->params.sample_phase == FR_SAMPLE_CENTER ? 1 : 0;
        return fr::launch_glyph_mask(e, a, st);
    }
    case fr::TL_CACHED: {
        fr::TextCachedArgs a = text_args<fr::TextCachedArgs>(plan, out_dev, out_stride);
        a.masks = plan->d_masks;
        return fr::launch_text_cached(e, a, st);
    }
    default:
        switch (e.form) {
        case fr::TEXT_AFFINE: return fr::launch_text(e, text_args<fr::TextAffineArgs>(plan, out_dev, out_stride), st);
        case fr::TEXT_EX: return fr::launch_text(e, text_args<fr::TextPlaceArgs>(plan, out_dev, out_stride), st);
        default: return fr::launch_text(e, text_args<fr::TextArgs>(plan, out_dev, out_stride), st);
        }
    }
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
    if (ctx->arena) (void)hipFree(ctx->arena);
    if (ctx->stage) (void)hipHostFree(ctx->stage);
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

int fr_ctx_set_option(fr_ctx *ctx, const char *key, int64_t value)
{
    if (!ctx || !key) return fail(FR_E_INVALID, "fr_ctx_set_option: NULL argument");
    ++ctx->opt_epoch;
    if (!strcmp(key, "graph")) { ctx->graph = value ? 1u : 0u; return FR_OK; }
    if (!strcmp(key, "kmax")) {
        if (value < 1 || value > 128) return fail(FR_E_INVALID, "kmax must be in [1,128]");
        ctx->kmax = (uint32_t)value;
        return FR_OK;
    }
    if (!strcmp(key, "strip_px")) {
        if (value < 16 || value > 256 || (value % 16)) return fail(FR_E_INVALID, "strip_px must be a multiple of 16 in [16,256]");
        ctx->strip_px = (uint32_t)value;
        return FR_OK;
    }
    if (!strcmp(key, "fuse_prepare")) { ctx->fuse_prepare = value ? 1u : 0u; return FR_OK; }
    if (!strcmp(key, "lds_pad")) { ctx->lds_pad = (uint32_t)value; return FR_OK; }
    if (!strcmp(key, "cov4")) { ctx->cov4 = value ? 1u : 0u; return FR_OK; }
    if (!strcmp(key, "row_cuts")) { ctx->row_cuts = value ? 1u : 0u; return FR_OK; }
    if (!strcmp(key, "sdf_cull")) { ctx->sdf_cull = value ? 1u : 0u; return FR_OK; }
    if (!strcmp(key, "overlap")) {
        if (value < 0 || value > 2) return fail(FR_E_INVALID, "overlap must be 0 (never), 1 (plans of >= 32 Mpixel) or 2 (always)");
        ctx->overlap = (uint32_t)value;
        return FR_OK;
    }
    if (!strcmp(key, "zero_copy")) { ctx->zero_copy = value ? 1u : 0u; return FR_OK; }
    if (!strcmp(key, "min_wgs")) {
        if (value < 1 || value > (1 << 24)) return fail(FR_E_INVALID, "min_wgs out of range");
        ctx->min_wgs = (uint32_t)value;
        return FR_OK;
    }
    return fail(FR_E_INVALID, "fr_ctx_set_option: unknown key '%s'", key);
}

// ---- glyph tables (flatten_segments and the two glyph bounds: fr_raster_plan.cpp) ---------------------------------------
void fr_glyphset_destroy(fr_glyphset *gs)
{
    if (!gs) return;
    (void)hipSetDevice(gs->ctx->device);
    (void)hipStreamSynchronize(gs->ctx->stream);
    dfree(gs->d_pts); dfree(gs->d_seg_pts); dfree(gs->d_seg_p0); dfree(gs->d_seg_prev); dfree(gs->d_glyph_seg_start);
    dfree(gs->d_rec_count); dfree(gs->d_recs); dfree(gs->d_seg_cut);
    delete gs;
}

int fr_glyphset_prepare(fr_glyphset *gs)
{
    if (!gs) return fail(FR_E_INVALID, "fr_glyphset_prepare: NULL");
    HIP_TRY(hipSetDevice(gs->ctx->device));
    fr::launch_prepare(gs->d_pts, gs->d_seg_p0, gs->d_glyph_seg_start, nullptr, gs->n_glyphs, gs->d_recs,
                       gs->d_rec_count, gs->ctx->stream);
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
    HIP_TRY(hipSetDevice(ctx->device));
    fr_glyphset *gs = new (std::nothrow) fr_glyphset;
    if (!gs) return fail(FR_E_NOMEM, "fr_glyphset_create: host allocation");
    gs->ctx = ctx; gs->n_glyphs = n_glyphs; gs->n_contours = n_contours;
    gs->n_seg = (uint32_t)seg_p0.size(); gs->n_points = np; gs->max_seg_per_glyph = max_seg;
    const size_t nseg1 = gs->n_seg ? gs->n_seg : 1, np1 = np ? np : 1;
#define GS_TRY(expr)                                                                          \
    do {                                                                                      \
        hipError_t e_ = (expr);                                                               \
        if (e_ != hipSuccess) {                                                               \
            fr_glyphset_destroy(gs);                                                          \
            return fail(e_ == hipErrorOutOfMemory ? FR_E_NOMEM : FR_E_HIP, "%s: %s", #expr,   \
                        hipGetErrorString(e_));                                               \
        }                                                                                     \
    } while (0)
    GS_TRY(hipMalloc(&gs->d_pts, np1 * 2 * sizeof(int16_t) + 16));
    GS_TRY(hipMalloc(&gs->d_seg_pts, nseg1 * 12 + 16));
    GS_TRY(hipMalloc(&gs->d_seg_p0, nseg1 * 4));
    GS_TRY(hipMalloc(&gs->d_seg_prev, nseg1 * 4));
    GS_TRY(hipMalloc(&gs->d_glyph_seg_start, ((size_t)n_glyphs + 1) * 4));
    GS_TRY(hipMalloc(&gs->d_rec_count, ((size_t)n_glyphs + 1) * 4));
    GS_TRY(hipMalloc(&gs->d_recs, 2 * nseg1 * sizeof(fr::Rec)));
    GS_TRY(hipMalloc(&gs->d_seg_cut, nseg1 * sizeof(float4)));
    hipStream_t st = ctx->stream;
    if (np) GS_TRY(hipMemcpyAsync(gs->d_pts, points_xy, np * 2 * sizeof(int16_t), hipMemcpyHostToDevice, st));
    std::vector<int16_t> seg_pts((size_t)gs->n_seg * 6);
    for (size_t sgi = 0; sgi < gs->n_seg; ++sgi) memcpy(&seg_pts[6 * sgi], points_xy + 2u * (size_t)seg_p0[sgi], 12);
    if (gs->n_seg) {
        GS_TRY(hipMemcpyAsync(gs->d_seg_pts, seg_pts.data(), (size_t)gs->n_seg * 12, hipMemcpyHostToDevice, st));
        GS_TRY(hipMemcpyAsync(gs->d_seg_p0, seg_p0.data(), (size_t)gs->n_seg * 4, hipMemcpyHostToDevice, st));
        GS_TRY(hipMemcpyAsync(gs->d_seg_prev, seg_prev.data(), (size_t)gs->n_seg * 4, hipMemcpyHostToDevice, st));
    }
    GS_TRY(hipMemcpyAsync(gs->d_glyph_seg_start, gseg.data(), ((size_t)n_glyphs + 1) * 4, hipMemcpyHostToDevice, st));
    gs->h_glyph_seg_start = gseg;
    gs->h_root_bound = root_bound;
    gs->h_ray_bound = ray_bound;
    GS_TRY(hipMemsetAsync(gs->d_rec_count, 0, ((size_t)n_glyphs + 1) * 4, st));
    fr::launch_prepare(gs->d_pts, gs->d_seg_p0, gs->d_glyph_seg_start, nullptr, n_glyphs, gs->d_recs,
                       gs->d_rec_count, st);
    GS_TRY(hipGetLastError());
    fr::launch_cuts(gs->d_seg_pts, gs->n_seg, gs->d_seg_cut, st);     // the row cuts: once, they hold for every cell and scale
    GS_TRY(hipGetLastError());
    GS_TRY(hipStreamSynchronize(st));   // host vectors above die with this frame
#undef GS_TRY
    *out = gs;
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
        HIP_TRY(hipMemcpy(cnt.data(), gs->d_rec_count, ((size_t)gs->n_glyphs) * 4, hipMemcpyDeviceToHost));
        uint64_t t = 0;
        for (uint32_t g = 0; g < gs->n_glyphs; ++g) t += cnt[g];
        *n_records = t;
    }
    return FR_OK;
}

// what a job must satisfy for the kernels' arithmetic to be the reference's (a plan's jobs, and the cells
// fr_selftest_row_cuts walks)
static int check_job(const fr_glyphset *gs, const fr_job &jb, uint32_t j)
{
    if (jb.glyph >= gs->n_glyphs) return fail(FR_E_INVALID, "job %u: glyph %u of %u", j, jb.glyph, gs->n_glyphs);
    if (!(jb.scale > 0.0f) || !std::isfinite(jb.scale)) return fail(FR_E_INVALID, "job %u: scale must be finite and > 0", j);
    // keeps every ray height, quotient and FMA residual of div_by_int inside the normal range
    // (the reference's own scale = u16 / u16 lies in [2^-16, 2^16])
    if (jb.scale < 9.5367431640625e-07f || jb.scale > 1048576.0f)
        return fail(FR_E_UNSUPPORTED, "job %u: scale outside [2^-20, 2^20]", j);
    if (jb.w > 65535u || jb.h > 65535u) return fail(FR_E_UNSUPPORTED, "job %u: cell larger than 65535", j);
    // sample coordinates must be exactly representable in binary32
    if (jb.min_x < -(1 << 22) || (int64_t)jb.min_x + jb.w > (1 << 22) || jb.max_y > (1 << 22) ||
        (int64_t)jb.max_y - jb.h < -(1 << 22))
        return fail(FR_E_UNSUPPORTED, "job %u: pixel coordinates beyond +-2^22", j);
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
    if (!gs->d_seg_cut) return fail(FR_E_INVALID, "fr_selftest_row_cuts: the glyph set has no row cuts");
    uint32_t max_rows = 0;
    for (uint32_t j = 0; j < n_jobs; ++j) {
        if (const int jrc = check_job(gs, jobs[j], j)) return jrc;
        max_rows = std::max(max_rows, jobs[j].h * (uint32_t)n);
    }
    *pairs = 0; *mismatches = 0;
    if (first_bad) first_bad[0] = first_bad[1] = first_bad[2] = 0u;
    if (n_jobs == 0 || max_rows == 0) return FR_OK;
    HIP_TRY(hipSetDevice(gs->ctx->device));
    hipStream_t st = gs->ctx->stream;
    fr::Job *d_jobs = nullptr;
    unsigned long long *d_res = nullptr;
    unsigned long long res[3] = {0ull, 0ull, ~0ull};
    hipError_t e = hipMalloc(&d_jobs, (size_t)n_jobs * sizeof(fr::Job));
    if (e == hipSuccess) e = hipMalloc(&d_res, sizeof res);
    if (e == hipSuccess) e = hipMemcpyAsync(d_jobs, jobs, (size_t)n_jobs * sizeof(fr::Job), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(d_res, res, sizeof res, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) {
        fr::launch_selftest_row_cuts(d_jobs, n_jobs, max_rows, gs->d_glyph_seg_start, gs->d_seg_pts, gs->d_seg_cut, n,
                                     phase == FR_SAMPLE_CENTER ? 1 : 0, d_res, st);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(res, d_res, sizeof res, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    else (void)hipStreamSynchronize(st);                  // (the copies above read `jobs` and `res`)
    dfree(d_jobs); dfree(d_res);
    if (e != hipSuccess) return fail(e == hipErrorOutOfMemory ? FR_E_NOMEM : FR_E_HIP, "fr_selftest_row_cuts: %s", hipGetErrorString(e));
    *pairs = res[0];
    *mismatches = res[1];
    if (first_bad && res[1]) {
        first_bad[0] = (uint32_t)(res[2] >> 40); first_bad[1] = (uint32_t)((res[2] >> 20) & 0xfffffu); first_bad[2] = (uint32_t)(res[2] & 0xfffffu);
    }
    return FR_OK;
}

// ---- plans ----------------------------------------------------------------
static int check_params(const fr_raster_params *p)
{
    if (!p) return fail(FR_E_INVALID, "params is NULL");
    if (p->mode < FR_WINDING_I16 || p->mode > FR_SDF_U8) return fail(FR_E_INVALID, "unknown mode %d", p->mode);
    const int n = p->samples_per_axis;
    if (p->mode == FR_COVERAGE_U8) {
        if (n != 1 && n != 2 && n != 4) return fail(FR_E_UNSUPPORTED, "samples_per_axis %d not in {1,2,4}", n);
    } else if (n != 1) {
        return fail(FR_E_INVALID, "samples_per_axis must be 1 for mode %d", p->mode);
    }
    if (p->sample_phase != FR_SAMPLE_CORNER && p->sample_phase != FR_SAMPLE_CENTER)
        return fail(FR_E_INVALID, "unknown sample_phase %d", p->sample_phase);
    return FR_OK;
}

void fr_plan_destroy(fr_plan *plan)
{
    if (!plan) return;
    (void)hipSetDevice(plan->ctx->device);
    (void)hipStreamSynchronize(plan->ctx->stream);
    dfree(plan->d_jobs); dfree(plan->d_job_seg); dfree(plan->d_large); dfree(plan->d_bits); dfree(plan->d_job_bits);
    dfree(plan->d_tiles); dfree(plan->d_runs); dfree(plan->d_insts); dfree(plan->d_tlist); dfree(plan->d_tglyphs);
    dfree(plan->d_trec_count); dfree(plan->d_trecs);
    dfree(plan->d_mcells); dfree(plan->d_mtiles); dfree(plan->d_masks);
    if (plan->ev0) (void)hipEventDestroy(plan->ev0);
    if (plan->ev1) (void)hipEventDestroy(plan->ev1);
    if (plan->gexec) (void)hipGraphExecDestroy(plan->gexec);
    delete plan;
}

// also: the bits an entry point takes besides FR_FILL_CONSISTENT (the RGBA text entry points: FR_TEXT_SRGB, FR_TEXT_BGRA,
// FR_TEXT_LOAD, FR_TEXT_OVER; the four upright and _ex text entry points: FR_TEXT_CACHE)
static int check_flags(uint32_t flags, uint32_t also = 0u)
{
    const uint32_t known = (uint32_t)FR_FILL_CONSISTENT | also;
    if (flags & ~known) return fail(FR_E_INVALID, "unknown flag bits 0x%x", flags & ~known);
    return FR_OK;
}

}  // extern "C"

// uploads the sorted jobs of raster_plan_build (fr_raster_plan.hpp), builds the other tables while that copy is under way
// (raster_plan_tables) and uploads them, into a plan that its caller destroys on failure
static int raster_plan_upload(fr_plan *p, const fr::RasterPlanIn &in, fr::RasterTables t)
{
    fr::RasterPlan &rp = p->rp;
    hipStream_t st = p->ctx->stream;
    hipError_t e = hipSetDevice(p->ctx->device);
    auto upload = [&](auto *&dst, const void *src, size_t bytes) {
        if (e != hipSuccess || !bytes) return;
        e = hipMalloc(&dst, bytes);
        if (e == hipSuccess) e = hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, st);
    };
    upload(p->d_jobs, t.sorted_jobs, (size_t)rp.n_jobs * sizeof(fr::Job));
    std::vector<uint32_t> jseg((size_t)rp.n_jobs * 2), large(rp.n_jobs - rp.n_fast), jbits(in.params.mode == FR_SDF_U8 ? rp.n_jobs : 0u);
    t.jseg = jseg.data(); t.large = large.data(); t.jbits = jbits.data();
    fr::raster_plan_tables(in, t, rp);
    upload(p->d_large, t.large, (size_t)rp.n_large * 4);
    upload(p->d_job_seg, t.jseg, (size_t)rp.n_jobs * 8);
    if (rp.bit_plane) {
        if (rp.bit_words >= 0xffffffffull) e = hipErrorInvalidValue;
        if (e == hipSuccess) e = hipMalloc(&p->d_bits, (size_t)(rp.bit_words ? rp.bit_words : 1) * 4);
        upload(p->d_job_bits, t.jbits, (size_t)rp.n_jobs * 4);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e == hipSuccess) e = hipEventCreate(&p->ev0);
    if (e == hipSuccess) e = hipEventCreate(&p->ev1);
    if (e != hipSuccess) return fail(e == hipErrorOutOfMemory ? FR_E_NOMEM : FR_E_HIP, "fr_plan_create: %s", hipGetErrorString(e));
    return FR_OK;
}

extern "C" {

int fr_plan_create(fr_ctx *ctx, const fr_glyphset *gs, const fr_job *jobs, uint32_t n_jobs,
                   const fr_raster_params *params, fr_plan **out)
{
    return fr_plan_create_ex(ctx, gs, jobs, n_jobs, params, 0u, out);
}

int fr_plan_create_ex(fr_ctx *ctx, const fr_glyphset *gs, const fr_job *jobs, uint32_t n_jobs,
                      const fr_raster_params *params, uint32_t flags, fr_plan **out)
{
    if (!ctx || !gs || !out) return fail(FR_E_INVALID, "fr_plan_create: NULL argument");
    *out = nullptr;
    if (const int frc = check_flags(flags)) return frc;
    if (gs->ctx != ctx) return fail(FR_E_INVALID, "glyph set belongs to another context");
    int rc = check_params(params);
    if (rc) return rc;
    if (n_jobs && !jobs) return fail(FR_E_INVALID, "jobs is NULL");
    for (uint32_t j = 0; j < n_jobs; ++j) {
        if (const int jrc = check_job(gs, jobs[j], j)) return jrc;
    }
    fr_plan *p = new (std::nothrow) fr_plan;
    if (!p) return fail(FR_E_NOMEM, "fr_plan_create: host allocation");
    p->ctx = ctx; p->gs = gs; p->params = *params; p->flags = flags;
    std::vector<uint8_t> cls(n_jobs);
    std::vector<uint32_t> order(n_jobs);
    std::vector<fr_job> sorted_jobs(n_jobs);
    const fr::RasterTables t = {cls.data(), order.data(), sorted_jobs.data(), nullptr, nullptr, nullptr};
    fr::RasterPlanIn in{};
    in.jobs = jobs; in.n_jobs = n_jobs; in.params = *params;
    in.glyph_seg_start = gs->h_glyph_seg_start.data(); in.root_bound = gs->h_root_bound.data(); in.ray_bound = gs->h_ray_bound.data();
    in.sdf_fast = true; in.merge = true; in.uniform = true;
    fr::raster_plan_build(in, raster_opts(ctx), t, p->rp);
    if (p->rp.too_many) {
        delete p;
        return fail(FR_E_UNSUPPORTED, "batch needs more than 2^31 workgroups; split it");
    }
    if (const int urc = raster_plan_upload(p, in, t)) {
        fr_plan_destroy(p);
        return urc;
    }
    *out = p;
    return FR_OK;
}

// ---- text runs (include/fr_raster.h) -----------------------------------------------------------
int fr_glyphset_set_boxes(fr_glyphset *gs, const int16_t *boxes)
{
    if (!gs || (gs->n_glyphs && !boxes)) return fail(FR_E_INVALID, "fr_glyphset_set_boxes: NULL argument");
    for (uint32_t g = 0; g < gs->n_glyphs; ++g)
        if (boxes[4 * (size_t)g] > boxes[4 * (size_t)g + 2] || boxes[4 * (size_t)g + 1] > boxes[4 * (size_t)g + 3])
            return fail(FR_E_INVALID, "glyph %u: box min above max", g);
    gs->h_box.assign(boxes, boxes + 4 * (size_t)gs->n_glyphs);
    return FR_OK;
}

}  // extern "C"

// uploads the tables of text_plan_tables (fr_text_plan.hpp) for a plan whose tp is set and that its caller destroys on
// failure
// `cache`: the tables of text_cache_tables for a plan that renders through its mask cells (else NULL)
template <class PLACE>
static int text_plan_upload(const char *fn, fr_plan *p, const fr::TextPlanTables<PLACE> &t, const fr::TextCacheTables *cache)
{
    fr_ctx *ctx = p->ctx;
    const fr_glyphset *gs = p->gs;
    p->rp.pixels = t.pixels; p->rp.need_cols = t.need_cols; p->rp.need_rows = t.need_rows;
    const bool recs = p->tp.n_glyphs != 0;
    hipStream_t st = ctx->stream;
    hipError_t e = hipSetDevice(ctx->device);
    auto upload = [&](auto *&dst, const auto &v) {
        using T = typename std::remove_reference<decltype(v)>::type::value_type;
        if (e != hipSuccess || v.empty()) return;
        e = hipMalloc(&dst, v.size() * sizeof(T));
        if (e == hipSuccess) e = hipMemcpyAsync(dst, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, st);
    };
    upload(p->d_tiles, t.tiles);
    upload(p->d_runs, t.runs);
    if (cache) {
        upload(p->d_insts, cache->insts);
        upload(p->d_mcells, cache->cells);
        upload(p->d_mtiles, cache->tiles);
        if (e == hipSuccess) e = hipMalloc(&p->d_masks, (size_t)cache->elems * sizeof(uint16_t));
    } else {
        upload(p->d_insts, t.insts);
    }
    upload(p->d_tlist, t.list);
    upload(p->d_tglyphs, t.glyphs);
    if (e == hipSuccess && recs) e = hipMalloc(&p->d_trecs, 2 * (size_t)gs->n_seg * sizeof(fr::Rec));
    if (e == hipSuccess && recs) e = hipMalloc(&p->d_trec_count, ((size_t)gs->n_glyphs + 1) * 4);
    if (e == hipSuccess && recs) e = hipMemsetAsync(p->d_trec_count, 0, ((size_t)gs->n_glyphs + 1) * 4, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e == hipSuccess) e = hipEventCreate(&p->ev0);
    if (e == hipSuccess) e = hipEventCreate(&p->ev1);
    if (e != hipSuccess) return fail(e == hipErrorOutOfMemory ? FR_E_NOMEM : FR_E_HIP, "%s: %s", fn, hipGetErrorString(e));
    return FR_OK;
}

// The six text entry points: the checks that need the context and the raster parameters, then the tables from
// text_plan_tables (fr_text_plan.cpp: plain host code, every check of the placements and runs and all the arithmetic),
// then text_plan_upload.  PLACE is the placement form: fr_glyph_place (TextInst, the text_* kernels of fr_text.hip),
// fr_glyph_place_ex (own scale, slant and sub-pixel baseline: TextInstEx, text_place_*) or fr_glyph_place_affine (a 2 x 2
// matrix: TextInstAffine, the text_affine_* kernels of fr_text_affine.hip).  rgba: place_rgba / run_clear_rgba are the
// colours (4 bytes each), the mode must be FR_COVERAGE_U8, the flags may add FR_TEXT_SRGB, FR_TEXT_BGRA,
// FR_TEXT_LOAD (which ignores run_clear_rgba and launches only the tiles some instance meets) and FR_TEXT_OVER (source-over
// alpha: blend = 2 when some placement colour is translucent).
// (The parameter checks are not check_params: that one answers FR_E_INVALID with other words for n != 1 outside
// coverage, and looks at n before the phase.)
template <class PLACE>
static int text_plan_create(const char *fn, fr_ctx *ctx, const fr_glyphset *gs, const PLACE *places, const uint8_t *place_rgba,
                            uint32_t n_places, const fr_text_run *runs, const uint8_t *run_clear_rgba, uint32_t n_runs,
                            const fr_raster_params *params, uint32_t flags, bool rgba, fr_plan **out)
{
    if (!ctx || !gs || !out) return fail(FR_E_INVALID, "%s: NULL argument", fn);
    *out = nullptr;
    constexpr bool can_cache = !std::is_same<PLACE, fr_glyph_place_affine>::value;
    if (const int frc = check_flags(flags, (rgba ? FR_TEXT_SRGB | FR_TEXT_BGRA | FR_TEXT_LOAD | FR_TEXT_OVER : 0u) | (can_cache ? FR_TEXT_CACHE : 0u))) return frc;
    if (gs->ctx != ctx) return fail(FR_E_INVALID, "glyph set belongs to another context");
    if (!params) return fail(FR_E_INVALID, "params is NULL");
    if (params->mode < FR_WINDING_I16 || params->mode > FR_SDF_U8) return fail(FR_E_INVALID, "unknown mode %d", params->mode);
    if (params->sample_phase != FR_SAMPLE_CORNER && params->sample_phase != FR_SAMPLE_CENTER)
        return fail(FR_E_INVALID, "unknown sample_phase %d", params->sample_phase);
    const int n = params->samples_per_axis;
    if (rgba) {
        if (params->mode != FR_COVERAGE_U8)
            return fail(FR_E_UNSUPPORTED, "RGBA text runs: mode %d (only FR_COVERAGE_U8)", params->mode);
        if (n != 1 && n != 2 && n != 4) return fail(FR_E_UNSUPPORTED, "RGBA text runs: samples_per_axis %d", n);
    } else {
        if (params->mode != FR_COVERAGE_U8 && params->mode != FR_MASK_NONZERO)
            return fail(FR_E_UNSUPPORTED, "text runs: mode %d has no meaning for overlapping instances", params->mode);
        if (params->mode == FR_COVERAGE_U8 ? (n != 1 && n != 2 && n != 4) : n != 1)
            return fail(FR_E_UNSUPPORTED, "text runs: samples_per_axis %d with mode %d", n, params->mode);
    }
    fr::TextPlanIn in{};
    in.runs = runs; in.n_runs = n_runs; in.n_places = n_places;
    in.place_rgba = place_rgba; in.run_clear_rgba = run_clear_rgba;
    in.rgba = rgba; in.flags = flags;
    in.boxes = gs->h_box.empty() ? nullptr : gs->h_box.data();
    in.glyph_seg_start = gs->h_glyph_seg_start.data(); in.n_glyphs = gs->n_glyphs;
    fr::TextPlanTables<PLACE> t;
    if (const int rc = fr::text_plan_tables(in, places, t)) return rc;
    // FR_TEXT_CACHE: the mask cells and the composite records (a plan whose placements are all clipped away has no cell
    // and stays the plan it is without the flag); the 2^31-element limit answers here, before anything is allocated
    fr::TextCacheTables cache;
    if constexpr (can_cache) {
        if (flags & FR_TEXT_CACHE)
            if (const int rc = fr::text_cache_tables(in, places, t, cache)) return rc;
    }

    fr_plan *p = new (std::nothrow) fr_plan;
    if (!p) return fail(FR_E_NOMEM, "%s: host allocation", fn);
    const fr::TextCacheTables *const cached = cache.cells.empty() ? nullptr : &cache;
    p->ctx = ctx; p->gs = gs; p->params = *params; p->flags = flags; p->text = true;
    p->tp = fr::text_plan_of(in, *params, t, cached);
    if (const int rc = text_plan_upload(fn, p, t, cached)) {
        fr_plan_destroy(p);
        return rc;
    }
    *out = p;
    return FR_OK;
}

extern "C" {

int fr_text_plan_create(fr_ctx *ctx, const fr_glyphset *gs, const fr_glyph_place *places, uint32_t n_places,
                        const fr_text_run *runs, uint32_t n_runs, const fr_raster_params *params, uint32_t flags,
                        fr_plan **out)
{
    return text_plan_create("fr_text_plan_create", ctx, gs, places, nullptr, n_places, runs, nullptr, n_runs, params, flags, false, out);
}
int fr_text_plan_create_rgba(fr_ctx *ctx, const fr_glyphset *gs, const fr_glyph_place *places, const uint8_t *place_rgba,
                             uint32_t n_places, const fr_text_run *runs, const uint8_t *run_clear_rgba, uint32_t n_runs,
                             const fr_raster_params *params, uint32_t flags, fr_plan **out)
{
    return text_plan_create("fr_text_plan_create_rgba", ctx, gs, places, place_rgba, n_places, runs, run_clear_rgba, n_runs, params, flags, true, out);
}
// the same two for fr_glyph_place_ex placements: own scale, slant and sub-pixel baseline per placement (the text_place_* kernels)
int fr_text_plan_create_ex(fr_ctx *ctx, const fr_glyphset *gs, const fr_glyph_place_ex *places, uint32_t n_places,
                           const fr_text_run *runs, uint32_t n_runs, const fr_raster_params *params, uint32_t flags,
                           fr_plan **out)
{
    return text_plan_create("fr_text_plan_create_ex", ctx, gs, places, nullptr, n_places, runs, nullptr, n_runs, params, flags, false, out);
}
int fr_text_plan_create_rgba_ex(fr_ctx *ctx, const fr_glyphset *gs, const fr_glyph_place_ex *places, const uint8_t *place_rgba,
                                uint32_t n_places, const fr_text_run *runs, const uint8_t *run_clear_rgba, uint32_t n_runs,
                                const fr_raster_params *params, uint32_t flags, fr_plan **out)
{
    return text_plan_create("fr_text_plan_create_rgba_ex", ctx, gs, places, place_rgba, n_places, runs, run_clear_rgba, n_runs, params, flags, true, out);
}
// the same two for fr_glyph_place_affine placements: a 2 x 2 matrix per placement (the text_affine_* kernels)
int fr_text_plan_create_affine(fr_ctx *ctx, const fr_glyphset *gs, const fr_glyph_place_affine *places, uint32_t n_places,
                               const fr_text_run *runs, uint32_t n_runs, const fr_raster_params *params, uint32_t flags,
                               fr_plan **out)
{
    return text_plan_create("fr_text_plan_create_affine", ctx, gs, places, nullptr, n_places, runs, nullptr, n_runs, params, flags, false, out);
}
int fr_text_plan_create_rgba_affine(fr_ctx *ctx, const fr_glyphset *gs, const fr_glyph_place_affine *places,
                                    const uint8_t *place_rgba, uint32_t n_places, const fr_text_run *runs,
                                    const uint8_t *run_clear_rgba, uint32_t n_runs, const fr_raster_params *params,
                                    uint32_t flags, fr_plan **out)
{
    return text_plan_create("fr_text_plan_create_rgba_affine", ctx, gs, places, place_rgba, n_places, runs, run_clear_rgba, n_runs, params, flags, true, out);
}

// the conversions of FR_TEXT_SRGB plans, from the tables text_srgb_kernel reads (fr_srgb.hpp)
int fr_srgb_decode(const uint8_t *in, size_t n, uint16_t *out)
{
    if (n && (!in || !out)) return fail(FR_E_INVALID, "fr_srgb_decode: NULL argument");
    for (size_t i = 0; i < n; ++i) out[i] = fr::SRGB_D[in[i]];
    return FR_OK;
}

int fr_srgb_encode(const uint16_t *in, size_t n, uint8_t *out)
{
    if (n && (!in || !out)) return fail(FR_E_INVALID, "fr_srgb_encode: NULL argument");
    for (size_t i = 0; i < n; ++i) {
        const uint32_t L = in[i], k = fr::SRGB_K[L >> 4];
        out[i] = (uint8_t)((k & 0xffu) + ((L & 15u) >= (k >> 8) ? 1u : 0u));
    }
    return FR_OK;
}

// premultiplied -> straight alpha, in place (the output of FR_TEXT_OVER plans; include/fr_raster.h)
int fr_rgba_unpremultiply(uint8_t *rgba, size_t n_pixels, int srgb)
{
    if (n_pixels && !rgba) return fail(FR_E_INVALID, "fr_rgba_unpremultiply: NULL argument");
    for (size_t i = 0; i < n_pixels; ++i) {
        uint8_t *p = rgba + 4 * i;
        const uint32_t a = p[3];
        if (a == 0u) { p[0] = p[1] = p[2] = 0; continue; }
        for (int c = 0; c < 3; ++c) {
            if (srgb) {
                const uint32_t L = std::min<uint32_t>(65535u, (255u * fr::SRGB_D[p[c]] + a / 2u) / a), k = fr::SRGB_K[L >> 4];
                p[c] = (uint8_t)((k & 0xffu) + ((L & 15u) >= (k >> 8) ? 1u : 0u));
            } else {
                p[c] = (uint8_t)std::min<uint32_t>(255u, (255u * p[c] + a / 2u) / a);
            }
        }
    }
    return FR_OK;
}

uint64_t fr_plan_pixels(const fr_plan *plan) { return plan ? plan->rp.pixels : 0; }

int fr_plan_stats(const fr_plan *plan, uint32_t *n_jobs_cov4, uint32_t *n_jobs_general)
{
    if (!plan) return fail(FR_E_INVALID, "fr_plan_stats: NULL");
    if (plan->text) {                  // every instance: text_kernel, a direct sum over the glyph's records (fr_text.hip)
        if (n_jobs_cov4) *n_jobs_cov4 = 0;
        if (n_jobs_general) *n_jobs_general = plan->tp.n_insts;
        return FR_OK;
    }
    if (n_jobs_cov4) *n_jobs_cov4 = plan->rp.n_fast;
    if (n_jobs_general) *n_jobs_general = plan->rp.n_jobs - plan->rp.n_fast;
    return FR_OK;
}

// the kernel instances a render of the plan launches, as rocprofv3 names them, with their job counts
int fr_plan_describe(const fr_plan *plan, char *buf, size_t cap)
{
    if (!plan || !buf || cap == 0) return fail(FR_E_INVALID, "fr_plan_describe: NULL argument");
    buf[0] = 0;
    size_t at = 0;
    auto add = [&](const char *name, uint32_t cnt) {
        const int k = snprintf(buf + at, cap - at, "%s%s x%u", at ? "; " : "", name, cnt);
        if (k > 0) at = std::min(cap - 1, at + (size_t)k);
    };
    char name[96];
    if (plan->text) {                  // the list a render walks (text_launch)
        fr::TextLaunchList L;
        fr::text_launches(plan->tp, L);
        for (uint32_t i = 0; i < L.n; ++i) {
            fr::text_launch_name(L.l[i], name, sizeof name);
            add(name, L.l[i].count);
        }
        return FR_OK;
    }
    fr::RasterLaunchList L;
    fr::raster_launches(plan->rp, plan->params, plan->flags, raster_opts(plan->ctx), plan->gs->max_seg_per_glyph, L);
    // (printed fast parts first, although a render launches the general kernel before them; prepare_kernel is not listed)
    for (const bool fast : {true, false})
        for (uint32_t i = 0; i < L.n; ++i) {
            const fr::RasterLaunch &e = L.l[i];
            if (e.family == fr::RL_PREPARE || (e.family == fr::RL_COV4 || e.family == fr::RL_WIN1) != fast) continue;
            fr::raster_launch_name(e, name, sizeof name);
            add(name, e.cnt);
        }
    return FR_OK;
}

static int ensure_aux(fr_ctx *ctx)
{
    if (!ctx->aux) {
        HIP_TRY(hipStreamCreateWithFlags(&ctx->aux, hipStreamNonBlocking));
        HIP_TRY(hipEventCreateWithFlags(&ctx->ev_fork, hipEventDisableTiming));
        HIP_TRY(hipEventCreateWithFlags(&ctx->ev_join, hipEventDisableTiming));
    }
    return FR_OK;
}

static int plan_check(fr_plan *plan, void *out_dev, size_t out_stride, size_t out_rows)
{
    if (!plan) return fail(FR_E_INVALID, "plan is NULL");
    // (a FR_TEXT_LOAD plan whose instances are all clipped away launches no tile, but its runs still need the output the
    // same plan with a visible glyph would: it is checked as that plan is)
    if (plan->rp.n_jobs == 0 && plan->tp.n_tiles == 0 && !(plan->tp.load && plan->rp.pixels)) return FR_OK;
    if (!out_dev) return fail(FR_E_INVALID, "out is NULL");
    if (plan->rp.need_cols > out_stride || plan->rp.need_rows > out_rows)
        return fail(FR_E_INVALID, "jobs need %llu x %llu elements, output is %zu x %zu",
                    (unsigned long long)plan->rp.need_cols, (unsigned long long)plan->rp.need_rows, out_stride, out_rows);
    // (the fast kernels address the rows of a wave band by 32-bit offsets from the band's base: 32 rows of the pitch)
    if (out_stride > ((size_t)1 << 26))
        return fail(FR_E_INVALID, "row pitch of %zu elements: at most 2^26", out_stride);
    if (plan->tp.rgba && ((uintptr_t)out_dev & 3u)) return fail(FR_E_INVALID, "RGBA output %p is not 4-byte aligned", out_dev);
    return FR_OK;
}

// one render of a text plan: the records of its glyphs from their points (plan-owned, so a plain plan's records are
// never touched), then text_kernel over every tile of every run — two launches in stream order, nothing to fork.
// An FR_TEXT_CACHE plan fills its mask cells from the records in between: three launches in stream order.  The list is the
// one fr_plan_describe prints (text_launches, fr_text_plan.hpp); a plan without tiles has an empty one
static int text_launch(fr_plan *plan, void *out_dev, size_t out_stride)
{
    fr::TextLaunchList L;
    fr::text_launches(plan->tp, L);
    if (L.n == 0) return FR_OK;
    HIP_TRY(hipSetDevice(plan->ctx->device));
    for (uint32_t i = 0; i < L.n; ++i) HIP_TRY(text_launch_entry(plan, L.l[i], out_dev, out_stride));
    return FR_OK;
}

// the launches of one render, issued on the context's stream(s)
static int plan_launch_direct(fr_plan *plan, void *out_dev, size_t out_stride, size_t out_rows)
{
    if (const int rc = plan_check(plan, out_dev, out_stride, out_rows)) return rc;
    if (plan->text) return text_launch(plan, out_dev, out_stride);
    if (plan->rp.n_jobs == 0) return FR_OK;
    HIP_TRY(hipSetDevice(plan->ctx->device));
    fr_ctx *const ctx = plan->ctx;
    fr::RasterLaunchList L;
    fr::raster_launches(plan->rp, plan->params, plan->flags, raster_opts(ctx), plan->gs->max_seg_per_glyph, L);
    const fr::RenderArgs a = render_args(plan, out_dev, out_stride);
    if (L.forked) {
        if (const int rc = ensure_aux(ctx)) return rc;
        HIP_TRY(hipEventRecord(ctx->ev_fork, ctx->stream));
        HIP_TRY(hipStreamWaitEvent(ctx->aux, ctx->ev_fork, 0));
    }
    auto run = [&](uint32_t i0, uint32_t i1, bool forked) -> int {
        for (uint32_t i = i0; i < i1; ++i)
            HIP_TRY(launch_entry(plan, a, L.l[i], (forked && !L.l[i].largest) ? ctx->aux : ctx->stream));
        return FR_OK;
    };
    // (whatever fails between the fork and the join: the context's stream still waits for the second one)
    const int rc_parts = run(0, L.join_at, L.forked);
    if (L.forked) {
        HIP_TRY(hipEventRecord(ctx->ev_join, ctx->aux));
        HIP_TRY(hipStreamWaitEvent(ctx->stream, ctx->ev_join, 0));
    }
    if (rc_parts) return rc_parts;
    return run(L.join_at, L.n, false);
}

// One render of a plan.  Option "graph": the same launches — the fork onto the second stream and the join included — are
// captured once per destination into a hipGraph and replayed with ONE hipGraphLaunch afterwards (the capture is redone when
// the destination or a context option changes).
static int plan_launch(fr_plan *plan, void *out_dev, size_t out_stride, size_t out_rows)
{
    if (const int rc = plan_check(plan, out_dev, out_stride, out_rows)) return rc;
    if (plan->rp.n_jobs == 0 && plan->tp.n_tiles == 0) return FR_OK;
    fr_ctx *const ctx = plan->ctx;
    if (!ctx->graph) return plan_launch_direct(plan, out_dev, out_stride, out_rows);
    HIP_TRY(hipSetDevice(ctx->device));
    if (plan->gexec && (plan->g_out != out_dev || plan->g_stride != out_stride || plan->g_rows != out_rows || plan->g_epoch != ctx->opt_epoch)) {
        (void)hipGraphExecDestroy(plan->gexec);
        plan->gexec = nullptr;
    }
    if (!plan->gexec) {
        if (const int rc = ensure_aux(ctx)) return rc;        // (nothing is created while the capture is open)
        HIP_TRY(hipStreamBeginCapture(ctx->stream, hipStreamCaptureModeRelaxed));
        const int rc = plan_launch_direct(plan, out_dev, out_stride, out_rows);
        hipGraph_t g = nullptr;
        const hipError_t ce = hipStreamEndCapture(ctx->stream, &g);
        if (rc) { if (g) (void)hipGraphDestroy(g); return rc; }
        HIP_TRY(ce);
        const hipError_t ie = hipGraphInstantiate(&plan->gexec, g, nullptr, nullptr, 0);
        (void)hipGraphDestroy(g);
        if (ie != hipSuccess) plan->gexec = nullptr;
        HIP_TRY(ie);
        plan->g_out = out_dev; plan->g_stride = out_stride; plan->g_rows = out_rows; plan->g_epoch = ctx->opt_epoch;
    }
    HIP_TRY(hipGraphLaunch(plan->gexec, ctx->stream));
    return FR_OK;
}

// ---- optional assembly over RCCL: bound at run time to the RCCL the host already uses (it created the communicator)
namespace {
using nccl_allgather_fn = int (*)(const void *, void *, size_t, int /* ncclDataType_t */, void * /* ncclComm_t */, hipStream_t);
using nccl_rank_fn = int (*)(void *, int *);
void *rccl_symbol(const char *name)
{
    if (void *p = dlsym(RTLD_DEFAULT, name)) return p;
    for (const char *lib : {"librccl.so", "librccl.so.1"})
        if (void *h = dlopen(lib, RTLD_NOW | RTLD_NOLOAD))            // only a library that is loaded already
            if (void *p = dlsym(h, name)) return p;
    return nullptr;
}
}  // namespace

int fr_allgather_bands(fr_ctx *ctx, void *nccl_comm, void *atlas_dev, size_t band_bytes)
{
    if (!ctx || !nccl_comm || !atlas_dev) return fail(FR_E_INVALID, "fr_allgather_bands: NULL argument");
    if (band_bytes == 0) return FR_OK;
    static const auto all_gather = reinterpret_cast<nccl_allgather_fn>(rccl_symbol("ncclAllGather"));
    static const auto user_rank = reinterpret_cast<nccl_rank_fn>(rccl_symbol("ncclCommUserRank"));
    if (!all_gather || !user_rank)
        return fail(FR_E_UNSUPPORTED, "fr_allgather_bands: no RCCL in this process (the host creates the communicator with it)");
    HIP_TRY(hipSetDevice(ctx->device));
    int rank = -1;
    if (user_rank(nccl_comm, &rank) != 0 || rank < 0) return fail(FR_E_INVALID, "fr_allgather_bands: ncclCommUserRank failed");
    const unsigned char *mine = static_cast<const unsigned char *>(atlas_dev) + (size_t)rank * band_bytes;
    const int rc = all_gather(mine, atlas_dev, band_bytes, 0 /* ncclInt8 / ncclChar */, nccl_comm, ctx->stream);
    if (rc != 0) return fail(FR_E_HIP, "fr_allgather_bands: ncclAllGather returned %d", rc);
    return FR_OK;
}

// Gather-to-root form of the same assembly (every peer has its own xGMI link to the root, so the root
// ingests up to 7 links' worth while no rank receives bytes it does not need — an all-gather moves W times the atlas):
// one RCCL group of point-to-point transfers — the root posts a receive per peer into that peer's slot of its atlas,
// every other rank one send of its own band.  root < 0: the all-gather above.
int fr_gather_bands(fr_ctx *ctx, void *nccl_comm, void *atlas_dev, size_t band_bytes, int root)
{
    if (root < 0) return fr_allgather_bands(ctx, nccl_comm, atlas_dev, band_bytes);
    if (!ctx || !nccl_comm || !atlas_dev) return fail(FR_E_INVALID, "fr_gather_bands: NULL argument");
    if (band_bytes == 0) return FR_OK;
    using p2p_fn = int (*)(void *, size_t, int, int, void *, hipStream_t);          // ncclSend / ncclRecv (buffer, count, type, peer, comm, stream)
    using group_fn = int (*)();
    using count_fn = int (*)(void *, int *);
    static const auto nsend = reinterpret_cast<p2p_fn>(rccl_symbol("ncclSend"));
    static const auto nrecv = reinterpret_cast<p2p_fn>(rccl_symbol("ncclRecv"));
    static const auto gstart = reinterpret_cast<group_fn>(rccl_symbol("ncclGroupStart"));
    static const auto gend = reinterpret_cast<group_fn>(rccl_symbol("ncclGroupEnd"));
    static const auto user_rank = reinterpret_cast<nccl_rank_fn>(rccl_symbol("ncclCommUserRank"));
    static const auto comm_count = reinterpret_cast<count_fn>(rccl_symbol("ncclCommCount"));
    if (!nsend || !nrecv || !gstart || !gend || !user_rank || !comm_count)
        return fail(FR_E_UNSUPPORTED, "fr_gather_bands: no RCCL in this process (the host creates the communicator with it)");
    HIP_TRY(hipSetDevice(ctx->device));
    int rank = -1, world = 0;
    if (user_rank(nccl_comm, &rank) != 0 || comm_count(nccl_comm, &world) != 0 || rank < 0 || world <= 0)
        return fail(FR_E_INVALID, "fr_gather_bands: ncclCommUserRank / ncclCommCount failed");
    if (root >= world) return fail(FR_E_INVALID, "fr_gather_bands: root %d of %d ranks", root, world);
    unsigned char *base = static_cast<unsigned char *>(atlas_dev);
    int rc = gstart();
    if (rc == 0) {
        if (rank == root) {
            for (int r = 0; r < world && rc == 0; ++r)
                if (r != root) rc = nrecv(base + (size_t)r * band_bytes, band_bytes, 0 /* ncclInt8 */, r, nccl_comm, ctx->stream);
        } else {
            rc = nsend(base + (size_t)rank * band_bytes, band_bytes, 0, root, nccl_comm, ctx->stream);
        }
        const int rc2 = gend();
        if (rc == 0) rc = rc2;
    }
    if (rc != 0) return fail(FR_E_HIP, "fr_gather_bands: RCCL returned %d", rc);
    return FR_OK;
}

int fr_plan_render(fr_plan *plan, void *out_dev, size_t out_stride, size_t out_rows)
{
    return plan_launch(plan, out_dev, out_stride, out_rows);
}

int fr_plan_render_timed(fr_plan *plan, void *out_dev, size_t out_stride, size_t out_rows, float *ms)
{
    if (!plan || !ms) return fail(FR_E_INVALID, "fr_plan_render_timed: NULL argument");
    HIP_TRY(hipSetDevice(plan->ctx->device));
    HIP_TRY(hipEventRecord(plan->ev0, plan->ctx->stream));
    int rc = plan_launch(plan, out_dev, out_stride, out_rows);
    if (rc) return rc;
    HIP_TRY(hipEventRecord(plan->ev1, plan->ctx->stream));
    HIP_TRY(hipEventSynchronize(plan->ev1));
    HIP_TRY(hipEventElapsedTime(ms, plan->ev0, plan->ev1));
    return FR_OK;
}

int fr_render_batch(fr_ctx *ctx, const fr_glyphset *gs, const fr_job *jobs, uint32_t n_jobs,
                    const fr_raster_params *params, void *out_host, size_t out_stride, size_t out_rows)
{
    return fr_render_batch_ex(ctx, gs, jobs, n_jobs, params, 0u, out_host, out_stride, out_rows);
}

int fr_render_batch_ex(fr_ctx *ctx, const fr_glyphset *gs, const fr_job *jobs, uint32_t n_jobs,
                       const fr_raster_params *params, uint32_t flags, void *out_host, size_t out_stride, size_t out_rows)
{
    fr_plan *plan = nullptr;
    int rc = fr_plan_create_ex(ctx, gs, jobs, n_jobs, params, flags, &plan);
    if (rc) return rc;
    if (n_jobs == 0) { fr_plan_destroy(plan); return FR_OK; }
    if (!out_host) { fr_plan_destroy(plan); return fail(FR_E_INVALID, "out_host is NULL"); }
    const size_t esz = params->mode == FR_WINDING_I16 ? 2 : 1;
    const size_t bytes = out_stride * out_rows * esz;
    void *d_out = nullptr;
    hipError_t e = hipMalloc(&d_out, bytes ? bytes : 16);
    // pixels outside every job keep the caller's bytes: stage the buffer in first
    if (e == hipSuccess) e = hipMemcpyAsync(d_out, out_host, bytes, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) {
        rc = plan_launch(plan, d_out, out_stride, out_rows);
        if (rc == FR_OK) {
            e = hipMemcpyAsync(out_host, d_out, bytes, hipMemcpyDeviceToHost, ctx->stream);
            if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        }
    }
    if (d_out) { (void)hipStreamSynchronize(ctx->stream); (void)hipFree(d_out); }
    fr_plan_destroy(plan);
    if (rc) return rc;
    if (e != hipSuccess) return fail(e == hipErrorOutOfMemory ? FR_E_NOMEM : FR_E_HIP, "fr_render_batch: %s", hipGetErrorString(e));
    return FR_OK;
}

// ---- renderGlyph drop-in ----------------------------------------------------
// render_glyph.zig:13-19, host arithmetic in binary32 exactly as written there.
int fr_render_glyph_dims(const int16_t box[4], uint16_t units_per_em, uint16_t font_size,
                         int16_t min_corner[2], int16_t max_corner[2], uint16_t *width,
                         uint16_t *height, float *scale_out)
{
    if (!box || !min_corner || !max_corner || !width || !height) return fail(FR_E_INVALID, "fr_render_glyph_dims: NULL argument");
    if (units_per_em == 0 || font_size == 0) return fail(FR_E_INVALID, "units_per_em and font_size must be > 0");
    const float scale = (float)font_size / (float)units_per_em;                    // :13
    const float b[4] = {(float)box[0] * scale, (float)box[1] * scale, (float)box[2] * scale, (float)box[3] * scale};   // :15
    const float lo0 = std::floor(b[0]), lo1 = std::floor(b[1]), hi0 = std::ceil(b[2]), hi1 = std::ceil(b[3]);
    if (lo0 < -32768.f || lo1 < -32768.f || hi0 > 32767.f || hi1 > 32767.f)
        return fail(FR_E_UNSUPPORTED, "scaled box leaves i16 (the reference's @intFromFloat would trap)");
    min_corner[0] = (int16_t)lo0; min_corner[1] = (int16_t)lo1;                    // :16
    max_corner[0] = (int16_t)hi0; max_corner[1] = (int16_t)hi1;                    // :17
    const int w = (int)max_corner[0] - min_corner[0] + 1, h = (int)max_corner[1] - min_corner[1] + 1;   // :18-19
    if (w < 1 || h < 1 || w > 32767 || h > 32767) return fail(FR_E_UNSUPPORTED, "image size leaves i16");
    *width = (uint16_t)w; *height = (uint16_t)h;
    if (scale_out) *scale_out = scale;
    return FR_OK;
}

// One glyph, one image — the reference's call shape.  No allocation per call: the glyph tables, the job and the
// output live in the context's device arena (grown on demand), filled by ONE host-to-device copy of a packed
// staging buffer; the render kernel builds the root records in LDS (prepare_kernel runs only for a glyph of
// more than 128 segments); the image comes back with one device-to-host copy.  The job covers the whole image,
// so the caller's buffer is never uploaded.
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
    if (const int frc = check_flags(flags)) return frc;
    int16_t mn[2], mx[2];
    uint16_t w, h;
    float scale;
    int rc = fr_render_glyph_dims(box, units_per_em, font_size, mn, mx, &w, &h, &scale);
    if (rc) return rc;
    fr_raster_params prm{};
    prm.mode = mode; prm.samples_per_axis = 1; prm.sample_phase = FR_SAMPLE_CORNER;
    rc = check_params(&prm);
    if (rc) return rc;
    if (!out_host) return fail(FR_E_INVALID, "out_host is NULL");
    const uint32_t zero_start[1] = {0};
    std::vector<uint32_t> seg_p0, seg_prev;
    uint64_t np = 0;
    rc = fr::flatten_segments(n_contours ? contour_start : zero_start, n_contours, &np, seg_p0, seg_prev, nullptr);
    if (rc) return rc;
    if (np && !points_xy) return fail(FR_E_INVALID, "points_xy is NULL");
    const uint32_t ns = (uint32_t)seg_p0.size();
    if (scale < 9.5367431640625e-07f || scale > 1048576.0f) return fail(FR_E_UNSUPPORTED, "scale outside [2^-20, 2^20]");
    fr_job jb{};
    jb.glyph = 0; jb.min_x = mn[0]; jb.max_y = mx[1]; jb.w = w; jb.h = h; jb.out_x = 0; jb.out_y = 0; jb.scale = scale;
    // arena layout (every part 16-byte aligned); the first `up` bytes are uploaded
    auto al = [](size_t v) { return (v + 15u) & ~(size_t)15; };
    const size_t esz = mode == FR_WINDING_I16 ? 2 : 1;
    const size_t o_pts = 0, o_p0 = al(o_pts + np * 4 + 16), o_spts = al(o_p0 + (size_t)ns * 4 + 4);
    const size_t o_gseg = al(o_spts + (size_t)ns * 12 + 16), o_job = al(o_gseg + 8), o_jseg = al(o_job + sizeof(fr_job));
    const size_t o_large = al(o_jseg + 8), up = al(o_large + 4);
    const size_t o_cnt = up, o_recs = al(o_cnt + 8), o_out = al(o_recs + (size_t)(ns ? ns : 1) * 2 * sizeof(fr::Rec));
    const size_t total = al(o_out + (size_t)w * h * esz);
    HIP_TRY(hipSetDevice(ctx->device));
    const size_t img_bytes = (size_t)w * h * esz;
    // Option "zero_copy" (off): the kernel reads the tables from, and writes the image to, the pinned staging block
    // itself (host memory mapped into the device's address space).  Measured on STIX 'A' in steady state: 34.9 us per
    // call against 34.7 us with the two small copies — no gain, so the copies stay the default.
    const bool zero_copy = ns <= 128u && mode != FR_SDF_U8 && total <= ((size_t)1 << 20) && ctx->zero_copy;
    if (!zero_copy && total > ctx->arena_cap) {
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        if (ctx->arena) { (void)hipFree(ctx->arena); ctx->arena = nullptr; ctx->arena_cap = 0; }
        const size_t cap = std::max<size_t>(total + total / 2, 1u << 20);
        HIP_TRY(hipMalloc(&ctx->arena, cap));
        ctx->arena_cap = cap;
    }
    const size_t stage_need = zero_copy ? total : up + img_bytes;
    if (stage_need > ctx->stage_cap) {
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        if (ctx->stage) { (void)hipHostFree(ctx->stage); ctx->stage = nullptr; ctx->stage_cap = 0; }
        const size_t cap = std::max<size_t>(stage_need * 2, 1u << 16);
        HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&ctx->stage), cap, hipHostMallocDefault));
        ctx->stage_cap = cap;
    }
    unsigned char *st = ctx->stage;
    memset(st, 0, up);
    if (np) memcpy(st + o_pts, points_xy, np * 4);
    if (ns) memcpy(st + o_p0, seg_p0.data(), (size_t)ns * 4);
    for (uint32_t sgi = 0; sgi < ns; ++sgi) memcpy(st + o_spts + 12u * (size_t)sgi, points_xy + 2u * (size_t)seg_p0[sgi], 12);
    const uint32_t gseg[2] = {0, ns}, jseg[2] = {0, ns}, large0[1] = {0};
    memcpy(st + o_gseg, gseg, 8); memcpy(st + o_job, &jb, sizeof jb); memcpy(st + o_jseg, jseg, 8); memcpy(st + o_large, large0, 4);
    unsigned char *A0 = zero_copy ? st : ctx->arena;
    if (!zero_copy) HIP_TRY(hipMemcpyAsync(A0, st, up, hipMemcpyHostToDevice, ctx->stream));
    // views of the arena dressed as a glyph set and a plan (nothing here owns memory: never destroyed)
    fr_glyphset gs;
    gs.ctx = ctx; gs.n_glyphs = 1; gs.n_contours = n_contours; gs.n_seg = ns; gs.max_seg_per_glyph = ns; gs.n_points = np;
    gs.d_pts = reinterpret_cast<int16_t *>(A0 + o_pts); gs.d_seg_pts = reinterpret_cast<int16_t *>(A0 + o_spts);
    gs.d_seg_p0 = reinterpret_cast<uint32_t *>(A0 + o_p0); gs.d_glyph_seg_start = reinterpret_cast<uint32_t *>(A0 + o_gseg);
    gs.d_rec_count = reinterpret_cast<uint32_t *>(A0 + o_cnt); gs.d_recs = reinterpret_cast<fr::Rec *>(A0 + o_recs);
    fr_plan pl;
    pl.ctx = ctx; pl.gs = &gs; pl.params = prm; pl.flags = flags;
    pl.d_jobs = reinterpret_cast<fr::Job *>(A0 + o_job); pl.d_job_seg = reinterpret_cast<uint32_t *>(A0 + o_jseg);
    pl.d_large = reinterpret_cast<uint32_t *>(A0 + o_large);
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
        fr::raster_plan_build(in, raster_opts(ctx), t1, pl.rp);
        fr::raster_plan_tables(in, t1, pl.rp);
    }
    int lrc = FR_OK;
    if (mode == FR_SDF_U8 || pl.rp.n_large) {
        // the stand-alone records (float brackets): the staged path of a large glyph and the SDF's stand-alone users
        hipError_t e = hipMemsetAsync(gs.d_rec_count, 0, 8, ctx->stream);
        if (e != hipSuccess) lrc = fail(FR_E_HIP, "hipMemsetAsync: %s", hipGetErrorString(e));
    }
    if (lrc == FR_OK) lrc = plan_launch_direct(&pl, A0 + o_out, w, h);
    hipError_t e = hipSuccess;
    if (lrc == FR_OK && !zero_copy) e = hipMemcpyAsync(st + up, A0 + o_out, img_bytes, hipMemcpyDeviceToHost, ctx->stream);
    hipError_t e2 = hipStreamSynchronize(ctx->stream);
    if (lrc == FR_OK && e == hipSuccess && e2 == hipSuccess) memcpy(out_host, zero_copy ? st + o_out : st + up, img_bytes);
    gs.d_pts = gs.d_seg_pts = nullptr; gs.d_seg_p0 = gs.d_glyph_seg_start = gs.d_rec_count = nullptr; gs.d_recs = nullptr;
    pl.d_jobs = nullptr; pl.d_job_seg = nullptr; pl.d_large = nullptr;
    if (lrc) return lrc;
    if (e == hipSuccess) e = e2;
    if (e != hipSuccess) return fail(FR_E_HIP, "fr_render_glyph: %s", hipGetErrorString(e));
    return FR_OK;
}

// ---- exact-integer path ---------------------------------------------------
struct ExactDev {
    int16_t *pts = nullptr;
    uint32_t *seg_p0 = nullptr, *seg_prev = nullptr;
    uint8_t *ctype = nullptr, *inc = nullptr;
    uint32_t n_seg = 0;
    int K = 1;
    ~ExactDev() { dfree(pts); dfree(seg_p0); dfree(seg_prev); dfree(ctype); dfree(inc); }
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
    HIP_TRY(hipMalloc(&d.pts, np1 * 4 + 16));
    HIP_TRY(hipMalloc(&d.seg_p0, ns1 * 4));
    HIP_TRY(hipMalloc(&d.seg_prev, ns1 * 4));
    HIP_TRY(hipMalloc(&d.ctype, ns1));
    HIP_TRY(hipMalloc(&d.inc, ns1));
    if (np) HIP_TRY(hipMemcpyAsync(d.pts, points_xy, np * 4, hipMemcpyHostToDevice, ctx->stream));
    if (d.n_seg) {
        HIP_TRY(hipMemcpyAsync(d.seg_p0, seg_p0.data(), (size_t)d.n_seg * 4, hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(hipMemcpyAsync(d.seg_prev, seg_prev.data(), (size_t)d.n_seg * 4, hipMemcpyHostToDevice, ctx->stream));
    }
    d.K = K;
    fr::launch_glyph_info(d.pts, d.seg_p0, d.seg_prev, d.n_seg, K, d.ctype, d.inc, ctx->stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return FR_OK;
}

int fr_glyph_info_init(fr_ctx *ctx, const int16_t *points_xy, const uint32_t *contour_start,
                       uint32_t n_contours, uint8_t *curve_type, uint8_t *include_p0)
{
    ExactDev d;
    int rc = exact_setup(ctx, points_xy, contour_start, n_contours, d);
    if (rc) return rc;
    if (d.n_seg) {
        if (!curve_type || !include_p0) return fail(FR_E_INVALID, "output is NULL");
        HIP_TRY(hipMemcpy(curve_type, d.ctype, d.n_seg, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(include_p0, d.inc, d.n_seg, hipMemcpyDeviceToHost));
    }
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
    int16_t *d_q = nullptr, *d_out = nullptr;
    hipError_t e = hipMalloc(&d_out, n_query * 2);
    if (e == hipSuccess && query_xy) e = hipMalloc(&d_q, n_query * 4);
    if (e == hipSuccess && query_xy) e = hipMemcpyAsync(d_q, query_xy, n_query * 4, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) {
        fr::launch_exact_winding(d.pts, d.seg_p0, d.ctype, d.inc, d.n_seg, d_q, n_query, lat_w, lat_x0, lat_y0, d.K, d_out, ctx->stream);
        e = hipGetLastError();
    }
    uint8_t *d_cov = nullptr;
    if (cover_n) {
        const size_t npx = (size_t)cover_w * cover_h;
        if (e == hipSuccess) e = hipMalloc(&d_cov, npx ? npx : 1);
        if (e == hipSuccess) {
            fr::launch_exact_cover(d_out, cover_w, cover_h, cover_n, d_cov, ctx->stream);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipMemcpyAsync(out_host, d_cov, npx, hipMemcpyDeviceToHost, ctx->stream);
    } else if (e == hipSuccess) {
        e = hipMemcpyAsync(out_host, d_out, n_query * 2, hipMemcpyDeviceToHost, ctx->stream);
    }
    hipError_t e2 = hipStreamSynchronize(ctx->stream);
    if (e == hipSuccess) e = e2;
    dfree(d_q); dfree(d_out); dfree(d_cov);
    if (e != hipSuccess) return fail(e == hipErrorOutOfMemory ? FR_E_NOMEM : FR_E_HIP, "exact winding: %s", hipGetErrorString(e));
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

// 128-bit predicates hold dy*abxy^2 < 2^106 * K^6 for i16 points scaled by K: K <= 8 cannot overflow
static int check_k(uint32_t K, int32_t x0, int32_t y0, uint64_t w, uint64_t h)
{
    if (K < 1 || K > 8) return fail(FR_E_UNSUPPORTED, "K must be in [1, 8] (128-bit predicate range)");
    if (w > (1u << 20) || h > (1u << 20)) return fail(FR_E_UNSUPPORTED, "lattice larger than 2^20 per axis");
    const int64_t lim = (int64_t)1 << 20;           // query points stay within a few em of the scaled glyph
    if (x0 < -lim || x0 + (int64_t)w > lim || y0 > lim || y0 - (int64_t)h < -lim)
        return fail(FR_E_UNSUPPORTED, "lattice beyond +-2^20 scaled units");
    return FR_OK;
}

int fr_exact_lattice(fr_ctx *ctx, const int16_t *points_xy, const uint32_t *contour_start,
                     uint32_t n_contours, uint32_t K, int32_t x0, int32_t y0, uint32_t w, uint32_t h,
                     int16_t *out_host)
{
    int rc = check_k(K, x0, y0, w, h);
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
    int rc = check_k(K, x0, y0, (uint64_t)w_px * n, (uint64_t)h_px * n);
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
    int16_t *d_lat = nullptr;
    uint8_t *d_rgb = nullptr;
    hipError_t e = hipMalloc(&d_lat, nq * 2);
    if (e == hipSuccess) e = hipMalloc(&d_rgb, nq * 3);
    if (e == hipSuccess) {
        // the lattice GlyphDebug.render walks (Image.zig:227-236), coloured on the device (setWindingLinear)
        fr::launch_exact_winding(d.pts, d.seg_p0, d.ctype, d.inc, d.n_seg, nullptr, nq, (uint32_t)W, box[0] - 1, box[3] + 1, 1, d_lat, ctx->stream);
        fr::launch_glyph_debug_color(d_lat, nq, winding_scale, 150u, d_rgb, ctx->stream);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(rgb_host, d_rgb, nq * 3, hipMemcpyDeviceToHost, ctx->stream);
    hipError_t e2 = hipStreamSynchronize(ctx->stream);
    if (e == hipSuccess) e = e2;
    dfree(d_lat); dfree(d_rgb);
    if (e != hipSuccess) return fail(e == hipErrorOutOfMemory ? FR_E_NOMEM : FR_E_HIP, "fr_glyph_debug_render: %s", hipGetErrorString(e));
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

int fr_atlas_layout(const int16_t *boxes, uint32_t n_glyphs, uint32_t first_glyph,
                    const uint16_t *units_per_em, uint32_t n_upm, uint16_t font_size,
                    uint32_t cell, uint32_t cols, uint32_t rows_per_page,
                    fr_job *jobs_out, uint32_t *page_of_job, uint32_t *n_pages)
{
    if (n_glyphs && (!boxes || !jobs_out)) return fail(FR_E_INVALID, "fr_atlas_layout: NULL argument");
    if (!units_per_em || (n_upm != 1 && n_upm != n_glyphs)) return fail(FR_E_INVALID, "units_per_em: one value or one per glyph");
    if (cell == 0 || cols == 0 || font_size == 0) return fail(FR_E_INVALID, "cell, cols and font_size must be > 0");
    if ((uint64_t)cell * cols > 0xffffffffull) return fail(FR_E_UNSUPPORTED, "atlas wider than 2^32 pixels");
    const uint64_t per_page = rows_per_page ? (uint64_t)rows_per_page * cols : 0;
    for (uint32_t i = 0; i < n_glyphs; ++i) {
        const uint16_t upm = units_per_em[n_upm == 1 ? 0 : i];
        if (upm == 0) return fail(FR_E_INVALID, "units_per_em must be > 0");
        const float scale = (float)font_size / (float)upm;                              // render_glyph.zig:13
        const float fx = std::floor((float)boxes[4 * (size_t)i + 0] * scale);           // :15-16
        const float fy = std::ceil((float)boxes[4 * (size_t)i + 3] * scale);            // :15, :17
        const uint64_t slot = per_page ? i % per_page : i;
        const uint64_t row = slot / cols;
        if (row * cell > 0xffffffffull) return fail(FR_E_UNSUPPORTED, "atlas taller than 2^32 pixels: use pages");
        fr_job &jb = jobs_out[i];
        jb.glyph = first_glyph + i;
        jb.min_x = (int32_t)fx; jb.max_y = (int32_t)fy;
        jb.w = cell; jb.h = cell;
        jb.out_x = (uint32_t)(slot % cols) * cell;
        jb.out_y = (uint32_t)row * cell;
        jb.scale = scale;
        if (page_of_job) page_of_job[i] = per_page ? (uint32_t)(i / per_page) : 0u;
    }
    if (n_pages) *n_pages = per_page ? (uint32_t)((n_glyphs + per_page - 1) / per_page) : (n_glyphs ? 1u : 0u);
    return FR_OK;
}

// renderGlyph's own image per glyph (render_glyph.zig:13-19 through fr_render_glyph_dims), shelf-packed in input order
int fr_atlas_layout_glyph_dims(const int16_t *boxes, uint32_t n_glyphs, uint32_t first_glyph,
                               const uint16_t *units_per_em, uint32_t n_upm, uint16_t font_size,
                               uint32_t atlas_w, uint32_t align, fr_job *jobs_out, uint32_t *atlas_h)
{
    if (n_glyphs && (!boxes || !jobs_out)) return fail(FR_E_INVALID, "fr_atlas_layout_glyph_dims: NULL argument");
    if (!units_per_em || (n_upm != 1 && n_upm != n_glyphs)) return fail(FR_E_INVALID, "units_per_em: one value or one per glyph");
    if (atlas_w == 0 || font_size == 0) return fail(FR_E_INVALID, "atlas_w and font_size must be > 0");
    if (align == 0) align = 1;
    uint64_t x = 0, y = 0, shelf_h = 0;
    for (uint32_t i = 0; i < n_glyphs; ++i) {
        int16_t mn[2], mx[2];
        uint16_t w, h;
        float scale;
        const int rc = fr_render_glyph_dims(boxes + 4 * (size_t)i, units_per_em[n_upm == 1 ? 0 : i], font_size, mn, mx, &w, &h, &scale);
        if (rc) return rc;
        if (w > atlas_w) return fail(FR_E_INVALID, "glyph %u is %u pixels wide, the atlas %u", i, (unsigned)w, atlas_w);
        x = (x + align - 1) / align * align;
        if (x + w > atlas_w) { x = 0; y += shelf_h; shelf_h = 0; }          // next shelf
        if (y + h > 0xffffffffull) return fail(FR_E_UNSUPPORTED, "atlas taller than 2^32 pixels");
        fr_job &jb = jobs_out[i];
        jb.glyph = first_glyph + i;
        jb.min_x = mn[0]; jb.max_y = mx[1];                                  // :26-27: sample (min_x + x, max_y - y)
        jb.w = w; jb.h = h;
        jb.out_x = (uint32_t)x; jb.out_y = (uint32_t)y;
        jb.scale = scale;
        x += w;
        shelf_h = std::max<uint64_t>(shelf_h, h);
    }
    if (atlas_h) *atlas_h = (uint32_t)std::min<uint64_t>(y + shelf_h, 0xffffffffull);
    return FR_OK;
}

}  // extern "C"

// fr_api_plan.hip — C ABI (include/fr_raster.h): plans of both kinds — create, launch (directly or as a captured graph),
// render, batch, describe.  What a plan launches is decided by plain C++ (fr_raster_plan.cpp, fr_text_plan.cpp); here the
// tables go to the device and the launch lists are walked over views of them.
#include "fr_internal.hpp"
#include "fr_text.hpp"

#include <cstdio>
#include <algorithm>
#include <new>
#include <type_traits>

namespace fr {
// fill = 1: the FR_FILL_CONSISTENT instances (fr_records.hpp)
void launch_prepare(const int16_t *, const uint32_t *, const uint32_t *, const uint32_t *, uint32_t, Rec *,
                    uint32_t *, hipStream_t, int fill = 0);
hipError_t launch_render(const RenderArgs &, const RasterLaunch &, hipStream_t);
uint32_t render_wg_waves();
hipError_t launch_cov4(const RenderArgs &, const RasterLaunch &, hipStream_t);
hipError_t launch_win1(const RenderArgs &, const RasterLaunch &, hipStream_t);
uint32_t cov4_wg_waves();
hipError_t launch_sdf(const RenderArgs &, uint32_t, uint32_t, uint32_t max_seg, int cull, hipStream_t);
}  // namespace fr

fr::RasterOpts raster_opts(const fr_ctx *ctx)
{
    return fr::RasterOpts{ctx->strip_px, ctx->cov4, ctx->fuse_prepare, ctx->min_wgs, ctx->overlap, fr::render_wg_waves(), fr::cov4_wg_waves(), ctx->kmax};
}

// ---- the launches of a raster render ----------------------------------------------------------------------------------
// what every launch of a raster render shares; launch_entry adds the entry's jobs and geometry
static fr::RenderArgs render_args(const fr_ctx *ctx, const GlyphView &g, const fr_raster_params &params, void *out_dev, size_t out_stride)
{
    fr::RenderArgs a{};
    a.glyph_seg_start = g.glyph_seg_start;
    a.glyph_rec_count = g.rec_count;
    a.recs = g.recs;
    a.pts = g.pts;
    a.seg_p0 = g.seg_p0;
    a.seg_pts = g.seg_pts;
    a.seg_cut = ctx->row_cuts ? g.seg_cut : nullptr;
    a.seg_cand = (ctx->row_cuts && ctx->cand_records) ? g.seg_cand : nullptr;
    // fused: the render kernel builds the records of every glyph of <= 128 segments (<= 256 candidate roots)
    // in LDS itself — decided per job inside the kernel; larger glyphs are staged from HBM
    a.fused = ctx->fuse_prepare ? 1u : 0u;
    a.out = out_dev;
    a.out_stride = out_stride;
    a.kmax = ctx->kmax;
    a.phase_center = params.sample_phase == FR_SAMPLE_CENTER ? 1 : 0;
    a.lds_pad = ctx->lds_pad;
    return a;
}

// one entry of a raster launch list (fr_raster_plan.hpp) on stream `st`
static hipError_t launch_entry(const fr_ctx *ctx, const GlyphView &g, const RasterView &r, const fr::RasterPlan &rp, fr::RenderArgs a,
                               const fr::RasterLaunch &e, hipStream_t st)
{
    a.jobs = r.jobs + e.first;
    a.job_seg = r.job_seg + 2u * (size_t)e.first;
    a.n_jobs = e.cnt; a.bands = e.bands; a.strips = e.strips; a.strip_w = e.strip_w; a.uniform = e.uniform ? 1u : 0u;
    a.bands_per_wg = e.bands_per_wg; a.band_groups = e.band_groups;
    switch (e.family) {
    case fr::RL_PREPARE:
        fr::launch_prepare(g.pts, g.seg_p0, g.glyph_seg_start, e.cnt ? r.large : nullptr, e.cnt ? e.cnt : g.n_glyphs, g.recs, g.rec_count, st, e.mode);
        return hipSuccess;
    case fr::RL_RENDER: return fr::launch_render(a, e, st);
    case fr::RL_COV4: return fr::launch_cov4(a, e, st);
    case fr::RL_WIN1:
        if (e.mode == 3) { a.out = r.bits; a.job_bits = r.job_bits + e.first; }     // the sign pass writes the bit planes
        return fr::launch_win1(a, e, st);
    default:                                                                                    // RL_SDF
        a.bits = r.bits; a.job_bits = r.job_bits;
        return fr::launch_sdf(a, rp.max_w, rp.max_h, g.max_seg_per_glyph, (int)ctx->sdf_cull, st);
    }
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

int raster_launch(fr_ctx *ctx, const GlyphView &g, const RasterView &r, const fr::RasterPlan &rp, const fr_raster_params &params,
                  uint32_t flags, void *out_dev, size_t out_stride)
{
    HIP_TRY(hipSetDevice(ctx->device));
    fr::RasterLaunchList L;
    fr::raster_launches(rp, params, flags, raster_opts(ctx), g.max_seg_per_glyph, L);
    const fr::RenderArgs a = render_args(ctx, g, params, out_dev, out_stride);
    if (L.forked) {
        if (const int rc = ensure_aux(ctx)) return rc;
        HIP_TRY(hipEventRecord(ctx->ev_fork, ctx->stream));
        HIP_TRY(hipStreamWaitEvent(ctx->aux, ctx->ev_fork, 0));
    }
    auto run = [&](uint32_t i0, uint32_t i1, bool forked) -> int {
        for (uint32_t i = i0; i < i1; ++i)
            HIP_TRY(launch_entry(ctx, g, r, rp, a, L.l[i], (forked && !L.l[i].largest) ? ctx->aux : ctx->stream));
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

// ---- the launches of a text render --------------------------------------------------------------------------------------
// the TextTables part of what a text kernel reads, over the instance table as the record type of ARGS (fr::TextArgs,
// fr::TextPlaceArgs, fr::TextAffineArgs or fr::TextCachedArgs, whose kernels do not read the records)
template <class ARGS>
static ARGS text_args(const TextView &v, const fr_raster_params &params, void *out_dev, size_t out_stride)
{
    ARGS a{};
    a.tiles = v.tiles; a.runs = v.runs; a.list = v.list;
    a.insts = static_cast<decltype(a.insts)>(v.insts);
    a.recs = v.recs; a.rec_count = v.rec_count;
    a.out = static_cast<uint8_t *>(out_dev);
    a.out_stride = out_stride;
    a.phase_center = params.sample_phase == FR_SAMPLE_CENTER ? 1 : 0;
    return a;
}

// one entry of a text launch list (fr_text_plan.hpp) on stream `st`
static hipError_t text_launch_entry(const GlyphView &g, const TextView &v, const fr_raster_params &params, const fr::TextLaunch &e,
                                    void *out_dev, size_t out_stride, hipStream_t st)
{
    switch (e.family) {
    case fr::TL_PREPARE:
        fr::launch_prepare(g.pts, g.seg_p0, g.glyph_seg_start, v.glyphs, e.grid, v.recs, v.rec_count, st, e.fill);
        return hipGetLastError();
    case fr::TL_MASK: {
        fr::TextMaskArgs a;
        a.tiles = v.mtiles; a.cells = v.mcells;
        a.recs = v.recs; a.rec_count = v.rec_count;
        a.masks = v.masks;
        a.phase_center = params.sample_phase == FR_SAMPLE_CENTER ? 1 : 0;
        return fr::launch_glyph_mask(e, a, st);
    }
    case fr::TL_CACHED: {
        fr::TextCachedArgs a = text_args<fr::TextCachedArgs>(v, params, out_dev, out_stride);
        a.masks = v.masks;
        return fr::launch_text_cached(e, a, st);
    }
    default:
        switch (e.form) {
        case fr::TEXT_AFFINE: return fr::launch_text(e, text_args<fr::TextAffineArgs>(v, params, out_dev, out_stride), st);
        case fr::TEXT_EX: return fr::launch_text(e, text_args<fr::TextPlaceArgs>(v, params, out_dev, out_stride), st);
        default: return fr::launch_text(e, text_args<fr::TextArgs>(v, params, out_dev, out_stride), st);
        }
    }
}

// ---- the two sides of a plan ---------------------------------------------------------------------------------------------
// Each owns its tables and offers the same four things about the plan `p` it belongs to: output_need (what a render asks
// of the destination), has_work, launch (the launches of one render) and describe (add(name, count) per kernel instance,
// as rocprofv3 names them) — and the two counts of fr_plan_stats.  with_side is the one place that picks.
struct OutputNeed {
    bool checked;                      // a render looks at the destination at all
    bool rgba;                         // which holds 4-byte pixels
};

struct RasterSide {
    // the job classes, the parts and the launch geometry (fr_raster_plan.hpp); jobs / job_seg hold the jobs in its order
    fr::RasterPlan rp;
    DevBuf<fr::Job> jobs;
    DevBuf<uint32_t> job_seg, large, bits, job_bits;

    RasterView view() const { return RasterView{jobs.get(), job_seg.get(), large.get(), bits.get(), job_bits.get()}; }
    OutputNeed output_need(const fr_plan &) const { return OutputNeed{rp.n_jobs != 0, false}; }
    bool has_work() const { return rp.n_jobs != 0; }
    void stats(uint32_t &fast, uint32_t &general) const { fast = rp.n_fast; general = rp.n_jobs - rp.n_fast; }
    int launch(const fr_plan &p, void *out_dev, size_t out_stride) const
    {
        return raster_launch(p.ctx, p.gs->view(), view(), rp, p.params, p.flags, out_dev, out_stride);
    }
    template <class ADD>
    void describe(const fr_plan &p, ADD add) const
    {
        char name[96];
        fr::RasterLaunchList L;
        fr::raster_launches(rp, p.params, p.flags, raster_opts(p.ctx), p.gs->max_seg_per_glyph, L);
        // (printed fast parts first, although a render launches the general kernel before them; prepare_kernel is not listed)
        for (const bool fast : {true, false})
            for (uint32_t i = 0; i < L.n; ++i) {
                const fr::RasterLaunch &e = L.l[i];
                if (e.family == fr::RL_PREPARE || (e.family == fr::RL_COV4 || e.family == fr::RL_WIN1) != fast) continue;
                fr::raster_launch_name(e, name, sizeof name);
                add(name, e.cnt);
            }
    }
};

struct TextSide {
    fr::TextPlan tp;                   // what its launches depend on (fr_text_plan.hpp)
    DevBuf<fr::TextTile> tiles;
    DevBuf<fr::TextRun> runs;
    DevBuf<unsigned char> insts, mcells;           // the records of tp.form (cached: TextCachedInst), and its mask cells
    DevBuf<uint32_t> list, glyphs, rec_count;
    DevBuf<fr::Rec> recs;
    DevBuf<fr::TextMaskTile> mtiles;
    DevBuf<uint16_t> masks;

    TextView view() const
    {
        return TextView{tiles.get(), runs.get(), insts.get(), list.get(), glyphs.get(), recs.get(), rec_count.get(), mcells.get(), mtiles.get(), masks.get()};
    }
    // (a FR_TEXT_LOAD plan whose instances are all clipped away launches no tile, but its runs still need the output the
    // same plan with a visible glyph would: it is checked as that plan is)
    OutputNeed output_need(const fr_plan &p) const { return OutputNeed{tp.n_tiles != 0 || (tp.load && p.pixels), tp.rgba}; }
    bool has_work() const { return tp.n_tiles != 0; }
    // every instance: a text kernel, a direct sum over the glyph's records (fr_text.hip)
    void stats(uint32_t &fast, uint32_t &general) const { fast = 0; general = tp.n_insts; }
    // One render: the records of its glyphs from their points (plan-owned, so a plain plan's records are never touched),
    // then the text kernel over every tile of every run — two launches in stream order, nothing to fork.  An FR_TEXT_CACHE or FR_TEXT_CACHE_AFFINE
    // plan fills its mask cells from the records in between: three launches in stream order.  A plan without tiles has
    // an empty list
    int launch(const fr_plan &p, void *out_dev, size_t out_stride) const
    {
        fr::TextLaunchList L;
        fr::text_launches(tp, L);
        if (L.n == 0) return FR_OK;
        HIP_TRY(hipSetDevice(p.ctx->device));
        const GlyphView g = p.gs->view();
        const TextView v = view();
        for (uint32_t i = 0; i < L.n; ++i) HIP_TRY(text_launch_entry(g, v, p.params, L.l[i], out_dev, out_stride, p.ctx->stream));
        return FR_OK;
    }
    template <class ADD>
    void describe(const fr_plan &, ADD add) const          // the list a render walks
    {
        char name[96];
        fr::TextLaunchList L;
        fr::text_launches(tp, L);
        for (uint32_t i = 0; i < L.n; ++i) {
            fr::text_launch_name(L.l[i], name, sizeof name);
            add(name, L.l[i].count);
        }
    }
};

template <class F>
static auto with_side(const fr_plan &p, F f) { return p.text ? f(*p.text) : f(*p.raster); }

fr_plan::fr_plan() = default;
fr_plan::~fr_plan()
{
    if (ctx) {
        (void)hipSetDevice(ctx->device);
        (void)hipStreamSynchronize(ctx->stream);
    }
    if (ev0) (void)hipEventDestroy(ev0);
    if (ev1) (void)hipEventDestroy(ev1);
    if (gexec) (void)hipGraphExecDestroy(gexec);
}

// the end of both uploads: the copies done (also after a failure: the host tables they read die with the callers' frames),
// then the events of fr_plan_render_timed
static int plan_finish(fr_plan *p, hipError_t e, const char *fn)
{
    const hipError_t es = hipStreamSynchronize(p->ctx->stream);
    if (e == hipSuccess) e = es;
    if (e == hipSuccess) e = hipEventCreate(&p->ev0);
    if (e == hipSuccess) e = hipEventCreate(&p->ev1);
    if (e != hipSuccess) return hip_fail(e, fn);
    return FR_OK;
}

// uploads the sorted jobs of raster_plan_build (fr_raster_plan.hpp), builds the other tables while that copy is under way
// (raster_plan_tables) and uploads them
static int raster_plan_upload(fr_plan *p, const fr::RasterPlanIn &in, fr::RasterTables t)
{
    RasterSide &s = *p->raster;
    fr::RasterPlan &rp = s.rp;
    hipStream_t st = p->ctx->stream;
    hipError_t e = hipSetDevice(p->ctx->device);
    s.jobs.upload(e, t.sorted_jobs, (size_t)rp.n_jobs * sizeof(fr::Job), st);
    std::vector<uint32_t> jseg((size_t)rp.n_jobs * 2), large(rp.n_jobs - rp.n_fast), jbits(in.params.mode == FR_SDF_U8 ? rp.n_jobs : 0u);
    t.jseg = jseg.data(); t.large = large.data(); t.jbits = jbits.data();
    fr::raster_plan_tables(in, t, rp);
    s.large.upload(e, t.large, (size_t)rp.n_large * 4, st);
    s.job_seg.upload(e, t.jseg, (size_t)rp.n_jobs * 8, st);
    if (rp.bit_plane) {
        if (rp.bit_words >= 0xffffffffull && e == hipSuccess) e = hipErrorInvalidValue;
        s.bits.alloc(e, (size_t)(rp.bit_words ? rp.bit_words : 1) * 4);
        s.job_bits.upload(e, t.jbits, (size_t)rp.n_jobs * 4, st);
    }
    return plan_finish(p, e, "fr_plan_create");       // (waits for the copies: jseg, large and jbits die here)
}

// uploads the tables of text_plan_tables (fr_text_plan.hpp) for a plan whose tp is set
// `cache`: the tables of text_cache_tables for a plan that renders through its mask cells (else NULL)
template <class PLACE>
static int text_plan_upload(const char *fn, fr_plan *p, const fr::TextPlanTables<PLACE> &t, const fr::TextCacheTables *cache)
{
    TextSide &s = *p->text;
    const fr_glyphset *gs = p->gs;
    p->pixels = t.pixels; p->need_cols = t.need_cols; p->need_rows = t.need_rows;
    const bool recs = s.tp.n_glyphs != 0;
    hipStream_t st = p->ctx->stream;
    hipError_t e = hipSetDevice(p->ctx->device);
    s.tiles.upload(e, t.tiles, st);
    s.runs.upload(e, t.runs, st);
    if (cache) {
        s.insts.upload(e, cache->insts, st);
        if constexpr (std::is_same<PLACE, fr_glyph_place_affine>::value) s.mcells.upload(e, cache->acells, st);
        else s.mcells.upload(e, cache->cells, st);
        s.mtiles.upload(e, cache->tiles, st);
        s.masks.alloc(e, (size_t)cache->elems * sizeof(uint16_t));
    } else {
        s.insts.upload(e, t.insts, st);
    }
    s.list.upload(e, t.list, st);
    s.glyphs.upload(e, t.glyphs, st);
    if (recs) {
        s.recs.alloc(e, 2 * (size_t)gs->n_seg * sizeof(fr::Rec));
        s.rec_count.alloc(e, ((size_t)gs->n_glyphs + 1) * 4);
        if (e == hipSuccess) e = hipMemsetAsync(s.rec_count.get(), 0, ((size_t)gs->n_glyphs + 1) * 4, st);
    }
    return plan_finish(p, e, fn);
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
    // (each form has its own cache flag, and answers FR_E_INVALID for the other's)
    constexpr uint32_t cache_flag = std::is_same<PLACE, fr_glyph_place_affine>::value ? FR_TEXT_CACHE_AFFINE : FR_TEXT_CACHE;
    if (const int frc = fr::check_flags(flags, (rgba ? FR_TEXT_SRGB | FR_TEXT_BGRA | FR_TEXT_LOAD | FR_TEXT_OVER : 0u) | cache_flag)) return frc;
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
    // FR_TEXT_CACHE, FR_TEXT_CACHE_AFFINE: the mask cells and the composite records (a plan whose placements are all clipped
    // away has no cell and stays the plan it is without the flag); the 2^31-element limit answers here, before anything is
    // allocated
    fr::TextCacheTables cache;
    if (flags & cache_flag)
        if (const int rc = fr::text_cache_tables(in, places, t, cache)) return rc;

    // (behind the tables: whatever fails in the upload, ~fr_plan waits for the copies that read them)
    std::unique_ptr<fr_plan> p(new (std::nothrow) fr_plan);
    if (p) p->text.reset(new (std::nothrow) TextSide);
    if (!p || !p->text) return fail(FR_E_NOMEM, "%s: host allocation", fn);
    const fr::TextCacheTables *const cached = cache.n_cells() ? &cache : nullptr;
    p->ctx = ctx; p->gs = gs; p->params = *params; p->flags = flags;
    p->text->tp = fr::text_plan_of(in, *params, t, cached);
    if (const int rc = text_plan_upload(fn, p.get(), t, cached)) return rc;
    *out = p.release();
    return FR_OK;
}

static int plan_check(const fr_plan *plan, void *out_dev, size_t out_stride, size_t out_rows)
{
    if (!plan) return fail(FR_E_INVALID, "plan is NULL");
    const OutputNeed need = with_side(*plan, [&](const auto &s) { return s.output_need(*plan); });
    if (!need.checked) return FR_OK;
    if (!out_dev) return fail(FR_E_INVALID, "out is NULL");
    if (plan->need_cols > out_stride || plan->need_rows > out_rows)
        return fail(FR_E_INVALID, "jobs need %llu x %llu elements, output is %zu x %zu",
                    (unsigned long long)plan->need_cols, (unsigned long long)plan->need_rows, out_stride, out_rows);
    // (the fast kernels address the rows of a wave band by 32-bit offsets from the band's base: 32 rows of the pitch)
    if (out_stride > ((size_t)1 << 26))
        return fail(FR_E_INVALID, "row pitch of %zu elements: at most 2^26", out_stride);
    if (need.rgba && ((uintptr_t)out_dev & 3u))
        return fail(FR_E_INVALID, "RGBA output %p is not 4-byte aligned", out_dev);
    return FR_OK;
}

// One render of a plan.  Option "graph": the same launches — the fork onto the second stream and the join included — are
// captured once per destination into a hipGraph and replayed with ONE hipGraphLaunch afterwards (the capture is redone when
// the destination or a context option that feeds a launch changes).
static int plan_launch(fr_plan *plan, void *out_dev, size_t out_stride, size_t out_rows)
{
    if (const int rc = plan_check(plan, out_dev, out_stride, out_rows)) return rc;
    const auto launch = [&] { return with_side(*plan, [&](const auto &s) { return s.has_work() ? s.launch(*plan, out_dev, out_stride) : (int)FR_OK; }); };
    fr_ctx *const ctx = plan->ctx;
    if (!ctx->graph || !with_side(*plan, [](const auto &s) { return s.has_work(); })) return launch();
    HIP_TRY(hipSetDevice(ctx->device));
    if (plan->gexec && (plan->g_out != out_dev || plan->g_stride != out_stride || plan->g_rows != out_rows || plan->g_epoch != ctx->opt_epoch)) {
        // (a replay of the stale graph may still be running, on both streams)
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        if (ctx->aux) HIP_TRY(hipStreamSynchronize(ctx->aux));
        (void)hipGraphExecDestroy(plan->gexec);
        plan->gexec = nullptr;
    }
    if (!plan->gexec) {
        if (const int rc = ensure_aux(ctx)) return rc;        // (nothing is created while the capture is open)
        HIP_TRY(hipStreamBeginCapture(ctx->stream, hipStreamCaptureModeRelaxed));
        const int rc = launch();
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

extern "C" {

void fr_plan_destroy(fr_plan *plan) { delete plan; }

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
    if (const int frc = fr::check_flags(flags)) return frc;
    if (gs->ctx != ctx) return fail(FR_E_INVALID, "glyph set belongs to another context");
    int rc = fr::check_params(params);
    if (rc) return rc;
    if (n_jobs && !jobs) return fail(FR_E_INVALID, "jobs is NULL");
    for (uint32_t j = 0; j < n_jobs; ++j) {
        if (const int jrc = fr::check_job(gs->n_glyphs, jobs[j], j)) return jrc;
    }
    std::vector<uint8_t> cls(n_jobs);
    std::vector<uint32_t> order(n_jobs);
    std::vector<fr_job> sorted_jobs(n_jobs);
    // (behind the tables: whatever fails in the upload, ~fr_plan waits for the copy that reads sorted_jobs)
    std::unique_ptr<fr_plan> p(new (std::nothrow) fr_plan);
    if (p) p->raster.reset(new (std::nothrow) RasterSide);
    if (!p || !p->raster) return fail(FR_E_NOMEM, "fr_plan_create: host allocation");
    p->ctx = ctx; p->gs = gs; p->params = *params; p->flags = flags;
    const fr::RasterTables t = {cls.data(), order.data(), sorted_jobs.data(), nullptr, nullptr, nullptr};
    fr::RasterPlanIn in{};
    in.jobs = jobs; in.n_jobs = n_jobs; in.params = *params;
    in.glyph_seg_start = gs->h_glyph_seg_start.data(); in.root_bound = gs->h_root_bound.data(); in.ray_bound = gs->h_ray_bound.data();
    in.sdf_fast = true; in.merge = true; in.uniform = true;
    fr::RasterPlan &rp = p->raster->rp;
    fr::raster_plan_build(in, raster_opts(ctx), t, rp);
    if (rp.too_many) return fail(FR_E_UNSUPPORTED, "batch needs more than 2^31 workgroups; split it");
    p->pixels = rp.pixels; p->need_cols = rp.need_cols; p->need_rows = rp.need_rows;
    if (const int urc = raster_plan_upload(p.get(), in, t)) return urc;
    *out = p.release();
    return FR_OK;
}

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

uint64_t fr_plan_pixels(const fr_plan *plan) { return plan ? plan->pixels : 0; }

int fr_plan_stats(const fr_plan *plan, uint32_t *n_jobs_cov4, uint32_t *n_jobs_general)
{
    if (!plan) return fail(FR_E_INVALID, "fr_plan_stats: NULL");
    uint32_t fast = 0, general = 0;
    with_side(*plan, [&](const auto &s) { s.stats(fast, general); return 0; });
    if (n_jobs_cov4) *n_jobs_cov4 = fast;
    if (n_jobs_general) *n_jobs_general = general;
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
    with_side(*plan, [&](const auto &s) { s.describe(*plan, add); return 0; });
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
    fr_plan *created = nullptr;
    int rc = fr_plan_create_ex(ctx, gs, jobs, n_jobs, params, flags, &created);
    if (rc) return rc;
    const std::unique_ptr<fr_plan> plan(created);
    if (n_jobs == 0) return FR_OK;
    if (!out_host) return fail(FR_E_INVALID, "out_host is NULL");
    const size_t esz = params->mode == FR_WINDING_I16 ? 2 : 1;
    const size_t bytes = out_stride * out_rows * esz;
    DevBuf<unsigned char> d_out;
    hipError_t e = hipSuccess;
    d_out.alloc(e, bytes ? bytes : 16);
    // pixels outside every job keep the caller's bytes: stage the buffer in first
    if (e == hipSuccess) e = hipMemcpyAsync(d_out.get(), out_host, bytes, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) {
        rc = plan_launch(plan.get(), d_out.get(), out_stride, out_rows);
        if (rc == FR_OK) {
            e = hipMemcpyAsync(out_host, d_out.get(), bytes, hipMemcpyDeviceToHost, ctx->stream);
            if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        }
    }
    if (d_out.get()) (void)hipStreamSynchronize(ctx->stream);
    if (rc) return rc;
    if (e != hipSuccess) return hip_fail(e, "fr_render_batch");
    return FR_OK;
}

}  // extern "C"

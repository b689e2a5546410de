// fr_raster_plan.cpp — the host rules of a raster plan (fr_raster_plan.hpp): plain host code, no HIP.
#include "fr_raster_plan.hpp"

#include <algorithm>
#include <cstdio>

namespace fr {

// ---- glyph tables --------------------------------------------------------
// Builds, per curve, the point index of its p0 and of the previous curve's p0 in the
// same contour (wrapping to the last curve: render_glyph.zig:126-127).
int flatten_segments(const uint32_t *contour_start, uint32_t n_contours, uint64_t *n_points,
                     std::vector<uint32_t> &seg_p0, std::vector<uint32_t> &seg_prev,
                     std::vector<uint32_t> *contour_seg_start)
{
    if (n_contours && !contour_start) return set_error(FR_E_INVALID, "contour_start is NULL");
    uint64_t np = n_contours ? contour_start[n_contours] : 0;
    if (n_contours && contour_start[0] != 0) return set_error(FR_E_INVALID, "contour_start[0] must be 0");
    if (contour_seg_start) contour_seg_start->assign(1, 0u);
    for (uint32_t c = 0; c < n_contours; ++c) {
        if (contour_start[c + 1] < contour_start[c]) return set_error(FR_E_INVALID, "contour_start not monotone at %u", c);
        const uint32_t len = contour_start[c + 1] - contour_start[c];
        // points.len = 2*curves + 1 (Glyph.zig:23); an even length would index past the
        // slice in the reference (render_glyph.zig:42)
        if (len != 0 && (len & 1u) == 0) return set_error(FR_E_INVALID, "contour %u has even length %u", c, len);
        const uint32_t curves = len / 2;                                    // render_glyph.zig:38
        for (uint32_t k = 0; k < curves; ++k) {
            seg_p0.push_back(contour_start[c] + 2 * k);
            seg_prev.push_back(contour_start[c] + (k != 0 ? 2 * k - 2 : len - 3));
        }
        if (contour_seg_start) contour_seg_start->push_back((uint32_t)seg_p0.size());
    }
    *n_points = np;
    return FR_OK;
}

// Upper bound of the root records a render can keep for a glyph (segments [s0, s1)): the two candidates of a segment
// minus those build_record_rows (fr_records.hpp) discards without looking at a cell — a == 0: one root, none if
// p2y == p0y (render_glyph.zig:49-50); else the far-side root when t_v = B/a >= 1 and the near-side root when t_v < 0.
uint32_t glyph_root_bound(const int16_t *points_xy, const uint32_t *seg_p0, uint32_t s0, uint32_t s1)
{
    uint32_t nb = 0;
    for (uint32_t sgi = s0; sgi < s1; ++sgi) {
        const int16_t *q = points_xy + 2u * (size_t)seg_p0[sgi];
        const int32_t p0y = q[1], p1y = q[3], p2y = q[5];
        const int32_t a = p0y - 2 * p1y + p2y, b = p0y - p1y;
        if (a == 0) { nb += (p2y != p0y) ? 1u : 0u; continue; }
        const int64_t ba = (int64_t)b * a;
        const bool tv_lt0 = ba < 0, tv_ge1 = a > 0 ? b >= a : b <= a;
        nb += (tv_ge1 ? 0u : 1u) + (tv_lt0 ? 0u : 1u);
    }
    return nb;
}

// Estimate of the most crossings one horizontal ray can have with a glyph: a sweep over the segments' y extents (the
// control points bound the curve), counted once between the heights of its ends and twice where it overshoots them.
// Glyphs that stay at or under 16 take the instance that keeps 16 crossings per sample row in registers (plan_classify).
// `ev` is scratch: (2 y + [closing], +-weight) — openings sort before closings at one y.
uint32_t glyph_ray_bound(const int16_t *points_xy, const uint32_t *seg_p0, uint32_t s0, uint32_t s1,
                         std::vector<std::pair<int32_t, int32_t>> &ev)
{
    ev.clear();
    for (uint32_t sgi = s0; sgi < s1; ++sgi) {
        const int16_t *q = points_xy + 2u * (size_t)seg_p0[sgi];
        const int32_t p0y = q[1], p1y = q[3], p2y = q[5];
        // between the heights of its two ends a quadratic is met once; where it overshoots them (towards the
        // control point: the vertex lies inside) twice, and not at all between the ends' heights on that side
        const int32_t clo = std::min(p0y, p2y), chi = std::max(p0y, p2y);
        // (half-open at the ends' heights, as the reference's own t in [0, 1) is: two segments that meet at a
        // vertex are not both counted there.  An estimate that steers jobs, not a proof: a row that does hold
        // more than the instance keeps takes the exact direct sum)
        ev.emplace_back(2 * clo, 1);
        ev.emplace_back(2 * chi, -1);
        // (the vertex overshoots the nearer end by at most half of what the control point does)
        if (p1y > chi) { ev.emplace_back(2 * chi, 2); ev.emplace_back(2 * (chi + (p1y - chi + 1) / 2) + 1, -2); }
        if (p1y < clo) { ev.emplace_back(2 * (clo - (clo - p1y + 1) / 2), 2); ev.emplace_back(2 * clo, -2); }
    }
    std::sort(ev.begin(), ev.end());
    int32_t cur = 0, best = 0;
    for (const auto &e : ev) { cur += e.second; best = std::max(best, cur); }
    return (uint32_t)best;
}

// Which kernel renders a job.  cov4_kernel (ns x ns samples, ns in {2, 4}) and win1_kernel (one sample per pixel)
// take cells of ANY width and height — renderGlyph's own image size (render_glyph.zig:14-19) included — up to 2048
// sample rows, of glyphs with <= 384 segments and <= 512 root records the vertex rule cannot discard: in strips of
// 64 / 128 / 256 pixels chosen from the job's own width (a 47 x 45 image does not pay for 256 columns) and bands of
// 64 sample rows, the last strip and band clipped at the cell's border.  Everything else takes the general
// render_kernel.  -> 0 (general) or 1 + 4 (wlog - 2) + record class (0: <= 128 slots and <= 16 crossings per ray
// estimated, 1: <= 256 slots, 2: <= 512 (<= 384 segments), 3: <= 1024 (<= 768 segments: two workgroups per CU)).
FastRule fast_rule(const RasterOpts &opt, const fr_raster_params *params)
{
    FastRule r;
    const int n = params->samples_per_axis;
    const bool one = params->mode == FR_WINDING_I16 || params->mode == FR_GRAY_DEBUG || params->mode == FR_MASK_NONZERO ||
                     (params->mode == FR_COVERAGE_U8 && n == 1) || params->mode == FR_SDF_U8;   // (SDF: its sign pass)
    r.wlog_max = opt.strip_px >= 256u ? 4u : (opt.strip_px >= 128u ? 3u : (opt.strip_px >= 64u ? 2u : 0u));
    if (opt.cov4 && r.wlog_max) r.ns = one ? 1 : ((params->mode == FR_COVERAGE_U8 && (n == 4 || n == 2)) ? n : 0);
    return r;
}
int fast_class(const FastRule &R, uint32_t w, uint32_t h, uint32_t nsg, uint32_t root_bound, uint32_t ray_bound)
{
    if (!R.ns || w == 0 || h == 0 || (uint64_t)h * (uint32_t)R.ns > 2048u) return 0;     // (12-bit sample-row fields)
    if (nsg > COV4_MAX_SEGMENTS || root_bound > 1024u) return 0;
    const uint32_t wl = std::min(w <= 64u ? 2u : (w <= 128u ? 3u : 4u), R.wlog_max);
    const int rc = (nsg <= 256u && root_bound <= 128u && ray_bound <= 16u) ? 0 : ((nsg <= 256u && root_bound <= 256u) ? 1 :
                   ((nsg <= 384u && root_bound <= 512u) ? 2 : 3));
    return 1 + FAST_RC * (int)(wl - 2u) + rc;
}
// classes of fewer than FAST_PART_MIN jobs move up into the next class that has jobs: same strip width and more record
// slots first, then wider strips with at least as many record slots (class c = 3 (wlog - 2) + record class; cls[j] = c + 1)
void merge_small_classes(uint32_t counts[FAST_CLASSES], uint8_t *cls, uint32_t n_jobs)
{
    int remap[FAST_CLASSES];
    bool any = false;
    for (int c = 0; c < FAST_CLASSES; ++c) {
        remap[c] = c;
        if (counts[c] == 0 || counts[c] >= (uint32_t)FAST_PART_MIN) continue;
        const int w = c / FAST_RC, r = c % FAST_RC;
        int target = -1;
        for (int w2 = w; w2 < 3 && target < 0; ++w2)
            for (int r2 = (w2 == w ? r + 1 : r); r2 < FAST_RC; ++r2)
                if (counts[FAST_RC * w2 + r2]) { target = FAST_RC * w2 + r2; break; }
        if (target < 0) continue;
        counts[target] += counts[c];          // (the target may be small itself: it is looked at later in this loop)
        counts[c] = 0;
        remap[c] = target;
        any = true;
    }
    if (!any) return;
    for (int c = 0; c < FAST_CLASSES; ++c) {             // chains: a -> b -> c
        int t = remap[c];
        while (remap[t] != t) t = remap[t];
        remap[c] = t;
    }
    for (uint32_t j = 0; j < n_jobs; ++j)
        if (cls[j]) cls[j] = (uint8_t)(remap[cls[j] - 1] + 1);
}

// the fast jobs of `order` (already grouped by class, `counts[c]` jobs of class c + 1) -> the plan's launches
static void make_parts(RasterPlan *p, const fr_job *sorted_jobs, const uint32_t counts[FAST_CLASSES], int ns)
{
    p->n_parts = 0;
    p->fast_ns = ns;
    if (ns <= 0) return;                                              // (no fast kernel in this plan)
    const uint32_t prb = ns == 1 ? 16u : 64u / (uint32_t)ns;          // pixel rows of a band
    uint32_t first = 0;
    for (int c = 0; c < FAST_CLASSES; ++c) {
        if (!counts[c]) continue;
        RasterPart pt{};
        pt.first = first; pt.cnt = counts[c]; pt.wlog = 2u + (uint32_t)(c / FAST_RC); pt.rec_cap = 128u << (c % FAST_RC);
        const uint32_t sw = 16u << pt.wlog;
        for (uint32_t q = first; q < first + counts[c]; ++q) {
            pt.bands = std::max(pt.bands, (sorted_jobs[q].h + prb - 1u) / prb);
            pt.strips = std::max(pt.strips, (sorted_jobs[q].w + sw - 1u) / sw);
            pt.pixels += (uint64_t)sorted_jobs[q].w * sorted_jobs[q].h;
        }
        p->parts[p->n_parts++] = pt;
        first += counts[c];
    }
}

void raster_plan_build(const RasterPlanIn &in, const RasterOpts &opt, const RasterTables &t, RasterPlan &p)
{
    const fr_job *jobs = in.jobs;
    const uint32_t n_jobs = in.n_jobs;
    const uint32_t n = (uint32_t)in.params.samples_per_axis;
    p = RasterPlan{};
    p.n_jobs = n_jobs;
    const uint32_t band = 64u / n;                                      // pixel rows per wave band
    const uint32_t cap_w = opt.strip_px;                                // strip width cap, pixels
    // Per JOB: the fast kernels or the general one (fast_class above).  The job table is stored fast jobs first, grouped
    // by class — one launch per class that occurs.
    uint32_t n_fast = 0;
    uint32_t counts[FAST_CLASSES] = {};
    const FastRule rule = fast_rule(opt, &in.params);
    {
        uint8_t *cls = t.cls;
        for (uint32_t j = 0; j < n_jobs; ++j) {
            const fr_job &jb = jobs[j];
            p.max_w = jb.w > p.max_w ? jb.w : p.max_w;
            p.max_h = jb.h > p.max_h ? jb.h : p.max_h;
            p.pixels += (uint64_t)jb.w * jb.h;
            p.need_cols = std::max<uint64_t>(p.need_cols, (uint64_t)jb.out_x + jb.w);
            p.need_rows = std::max<uint64_t>(p.need_rows, (uint64_t)jb.out_y + jb.h);
            const uint32_t nsg = in.glyph_seg_start[jb.glyph + 1] - in.glyph_seg_start[jb.glyph];
            cls[j] = (uint8_t)fast_class(rule, jb.w, jb.h, nsg, in.root_bound[jb.glyph], in.ray_bound[jb.glyph]);
            if (in.params.mode == FR_SDF_U8 && !in.sdf_fast) cls[j] = 0;   // (one SDF image: the sign comes as a byte from the general kernel, no bit plane)
            if (cls[j]) { ++counts[cls[j] - 1]; ++n_fast; }
        }
        // A class with only a handful of jobs is not worth a launch of its own (a real font at renderGlyph's sizes: three or
        // four glyphs per odd class, each launch a few microseconds on the second stream): its jobs join the next class up
        // that exists — wider strips and / or more record slots render the same bytes (the stores are clipped, spare
        // record slots stay empty), only a little less efficiently.
        if (in.merge) merge_small_classes(counts, cls, n_jobs);
        uint32_t at[FAST_CLASSES + 1], run = 0;
        for (int c = 0; c < FAST_CLASSES; ++c) { at[c + 1] = run; run += counts[c]; }
        at[0] = run;                                                      // the general kernel's jobs go last
        for (uint32_t j = 0; j < n_jobs; ++j) t.order[at[cls[j]]++] = j;
    }
    const uint32_t *order = t.order;
    p.n_fast = n_fast;
    // the general list: uniform = every strip of every job is full (w a multiple of the strip width) and every wave
    // band is full (h a multiple of 64 / n pixel rows) — atlas cells; the render kernel has instances for it
    p.uniform = in.uniform && n_jobs > n_fast;
    uint32_t gmax_w = 0, gmax_h = 0;
    for (uint32_t q = n_fast; q < n_jobs; ++q) {
        gmax_w = std::max(gmax_w, jobs[order[q]].w); gmax_h = std::max(gmax_h, jobs[order[q]].h);
    }
    uint32_t sw = (gmax_w + 15u) & ~15u;                                // the general kernel's strip width
    if (sw > cap_w) sw = cap_w;
    if (sw == 0) sw = 16;
    p.strip_w = sw;
    for (uint32_t q = n_fast; q < n_jobs; ++q) {
        const fr_job &jb = jobs[order[q]];
        if (jb.w == 0 || jb.h == 0 || jb.w % sw || jb.h % band) p.uniform = false;
    }
    p.gen_bands = gmax_h ? (gmax_h + band - 1) / band : 1;
    p.gen_strips = gmax_w ? (gmax_w + sw - 1) / sw : 1;
    fr_job *sorted_jobs = t.sorted_jobs;
    for (uint32_t q = 0; q < n_jobs; ++q) sorted_jobs[q] = jobs[order[q]];
    make_parts(&p, sorted_jobs, counts, rule.ns);
    p.too_many = (uint64_t)(n_jobs - n_fast) * p.gen_bands * p.gen_strips > 0x7fffffffull;
    for (uint32_t i = 0; i < p.n_parts; ++i)
        p.too_many = p.too_many || (uint64_t)p.parts[i].cnt * p.parts[i].bands * p.parts[i].strips > 0x7fffffffull;
}

void raster_plan_tables(const RasterPlanIn &in, const RasterTables &t, RasterPlan &p)
{
    const uint32_t n_jobs = p.n_jobs, n_fast = p.n_fast;
    const fr_job *sorted_jobs = t.sorted_jobs;
    // each job's segment range, next to the job: the render kernel starts on the glyph's points without a
    // dependent look-up through the glyph table
    uint32_t *jseg = t.jseg;
    for (uint32_t q = 0; q < n_jobs; ++q) {
        const uint32_t gl = sorted_jobs[q].glyph;
        jseg[2 * (size_t)q] = in.glyph_seg_start[gl];
        jseg[2 * (size_t)q + 1] = in.glyph_seg_start[gl + 1] - in.glyph_seg_start[gl];
    }
    // glyphs too large for the in-kernel record build (> 128 segments) among the general kernel's jobs, each once
    uint32_t nl = 0;
    for (uint32_t q = n_fast; q < n_jobs; ++q)
        if (jseg[2 * (size_t)q + 1] > 128u) t.large[nl++] = sorted_jobs[q].glyph;
    std::sort(t.large, t.large + nl);
    p.n_large = (uint32_t)(std::unique(t.large, t.large + nl) - t.large);
    // FR_SDF_U8: the sign of a fast job travels as one bit per pixel in a plane of its own (win1_kernel's sign-bit mode
    // writes it, sdf_kernel reads it and is then the only writer of the output)
    if (in.params.mode == FR_SDF_U8 && n_fast) {
        p.bit_plane = true;
        std::fill(t.jbits, t.jbits + n_jobs, 0xffffffffu);
        uint64_t words = 0;
        for (uint32_t q = 0; q < n_fast; ++q) {
            t.jbits[q] = (uint32_t)words;
            words += (uint64_t)((sorted_jobs[q].w + 255u) / 256u) * sorted_jobs[q].h * 8u;      // (one plane per 256-pixel column: h rows of 8 words)
            if (words >= 0xffffffffull) break;
        }
        p.bit_words = words;
    }
}

std::pair<uint32_t, uint32_t> split_bands(uint32_t nw, uint32_t njobs, uint32_t bands, uint32_t strips, uint32_t min_wgs)
{
    // (bands are wave bands of 64/n pixel rows; a workgroup's waves take them round-robin)
    uint32_t bpw = (bands + nw - 1u) / nw * nw;
    while (bpw > nw && (uint64_t)njobs * strips * ((bands + bpw - 1) / bpw) < min_wgs) bpw = ((bpw / 2) + nw - 1u) / nw * nw;
    return {bpw, (bands + bpw - 1) / bpw};
}

void raster_launches(const RasterPlan &p, const fr_raster_params &params, uint32_t flags, const RasterOpts &opt, uint32_t max_seg,
                     RasterLaunchList &out)
{
    out.n = out.join_at = 0;
    out.forked = false;
    if (p.n_jobs == 0) return;
    const uint32_t n_gen = p.n_jobs - p.n_fast;
    const int pm = params.mode;
    const bool sdf = pm == FR_SDF_U8;
    const int fill = (flags & FR_FILL_CONSISTENT) ? 1 : 0;
    auto push = [&](RasterFamily f, int mode, int samples, uint32_t first, uint32_t cnt) -> RasterLaunch & {
        RasterLaunch &e = out.l[out.n++];
        e = RasterLaunch{};
        e.family = f; e.mode = mode; e.samples = samples; e.first = first; e.cnt = cnt; e.fill = fill != 0;
        return e;
    };
    auto instance = [](RasterLaunch &e, int a, int b, int c, int d) { e.targ[0] = a; e.targ[1] = b; e.targ[2] = c; e.targ[3] = d; };
    // crossings a sample row keeps in registers before it takes the direct sum: option kmax -> CAP
    auto cap_of = [](uint32_t kmax) { return kmax <= 8u ? 8 : (kmax <= 16u ? 16 : 32); };
    auto geometry = [&](RasterLaunch &e, uint32_t nw, uint32_t strip_w, uint32_t bands, uint32_t strips, bool uniform) {
        e.strip_w = strip_w; e.bands = bands; e.strips = strips; e.uniform = uniform;
        const auto s = split_bands(nw, e.cnt, bands, strips, opt.min_wgs);
        e.bands_per_wg = s.first; e.band_groups = s.second;
    };
    // A mixed plan: the smaller launches (a real font's few glyphs of many segments: the 512-record instance, the
    // general kernel) are short kernels with long critical paths — forked onto a second stream so that they run beside
    // the large one instead of before / after it (the jobs' cells are disjoint); joined before anything else touches the
    // output.
    // (a small plan — a font at renderGlyph's own sizes for one font size: a few megapixels — is quicker launch after launch
    // on one stream than through a fork and a join: measured 0.038 vs 0.056 ms at 5.8 Mpixel, 0.373 vs 0.356 at 221 Mpixel)
    const uint32_t n_launches = (n_gen ? 1u : 0u) + p.n_parts;
    out.forked = opt.overlap && p.n_fast && n_launches > 1 && (opt.overlap == 2u || p.pixels >= ((uint64_t)32 << 20));
    // a render always starts from the glyph POINTS: inside the kernels (fused) or by re-running the stand-alone
    // precompute first, for the glyphs that need it
    // (FR_FILL_CONSISTENT: its own records, the reference's are rebuilt behind the render: the glyph set's records and
    // counts are the reference's outside a render, fr_glyphset_stats included)
    auto prepare = [&](int f) {
        if (n_gen && !opt.fuse_prepare) push(RL_PREPARE, f, 0, 0, 0);
        else if (n_gen && p.n_large) push(RL_PREPARE, f, 0, 0, p.n_large);
    };
    prepare(fill);
    if (n_gen) {
        // SDF, sign first: the 1-sample coverage (255 where the reference's winding is non-zero, same sample points)
        // lands in the output; the distance kernel reads it and overwrites it
        RasterLaunch &e = push(RL_RENDER, sdf ? (int)FR_COVERAGE_U8 : pm, sdf ? 1 : params.samples_per_axis, p.n_fast, n_gen);
        geometry(e, opt.render_waves, p.strip_w, p.gen_bands, p.gen_strips, p.uniform);
        // winding != 0 ? 255 : 0 is exactly the 1-sample coverage (round_half_up(255 k / 1), k in {0, 1}); uniform plans of
        // 256- / 128-pixel strips (atlas cells) at 4 x 4 samples take the specialised instances
        const bool cov = e.mode == FR_COVERAGE_U8;
        const int wlog = (cov && e.samples == 4 && e.uniform) ? (e.strip_w == 256u ? 4 : (e.strip_w == 128u ? 3 : -1)) : -1;
        const int kmode = (e.mode == FR_MASK_NONZERO && e.samples == 1) ? (int)FR_COVERAGE_U8 : e.mode;
        instance(e, kmode, e.samples, cap_of(opt.kmax), wlog);
        if (fill) prepare(0);
    }
    // (the largest fast launch stays on the context's stream; every other launch of the plan goes beside it)
    uint32_t big = 0;
    for (uint32_t i = 1; i < p.n_parts; ++i)
        if (p.parts[i].pixels > p.parts[big].pixels) big = i;
    for (uint32_t i = 0; i < p.n_parts; ++i) {
        // cov4_kernel / win1_kernel, one launch per (strip width, record slots) class that occurs in the plan; FR_SDF_U8: the
        // sign pass, one bit per pixel into the job's own bit plane
        const RasterPart &pt = p.parts[i];
        const int m1 = pm == FR_WINDING_I16 ? 0 : (pm == FR_GRAY_DEBUG ? 1 : (sdf ? 3 : 2));
        RasterLaunch &e = p.fast_ns > 1 ? push(RL_COV4, 0, p.fast_ns, pt.first, pt.cnt) : push(RL_WIN1, m1, 1, pt.first, pt.cnt);
        e.rec_cap = pt.rec_cap; e.largest = i == big;
        geometry(e, opt.fast_waves, 16u << pt.wlog, pt.bands, pt.strips, true);
        // root records per lane: 64 RPL record slots
        const int rpl = pt.rec_cap <= 128u ? 2 : (pt.rec_cap <= 256u ? 4 : (pt.rec_cap > 512u ? 16 : 8));
        if (e.family == RL_WIN1) { instance(e, (int)pt.wlog, e.mode, rpl, 0); continue; }
        // glyphs of <= 128 candidate roots (RPL == 2) all but never put more than 16 crossings on a sample row (a real font:
        // 1 row in 100 000): their instance keeps 16 per row in registers — half the list to initialise, pull and sort, 5 %
        // faster — and the rare fuller row takes the direct sum like any over-full row
        // (the 1024-record instance — glyphs of 385 .. 768 segments, rare — exists with 32 kept crossings only)
        const int cap = rpl >= 16 ? 32 : cap_of((rpl == 2 && opt.kmax > 16u) ? 16u : opt.kmax);
        instance(e, (int)pt.wlog, cap, rpl, e.samples);
    }
    out.join_at = out.n;
    if (sdf) {
        RasterLaunch &e = push(RL_SDF, max_seg > 64u ? 1 : 0, 0, 0, p.n_jobs);
        e.strip_w = p.strip_w; e.targ[0] = e.mode;
    }
}

void raster_launch_name(const RasterLaunch &e, char *name, size_t cap)
{
    const int *t = e.targ;
    const char *tail = e.fill ? ", 1>" : ">";
    switch (e.family) {
    case RL_RENDER: snprintf(name, cap, "fr::render_kernel<%d, %d, %d, %d%s", t[0], t[1], t[2], t[3], tail); break;
    case RL_COV4: snprintf(name, cap, "fr::cov4_kernel<%d, %d, %d, %d%s", t[0], t[1], t[2], t[3], tail); break;
    case RL_WIN1: snprintf(name, cap, "fr::win1_kernel<%d, %d, %d%s", t[0], t[1], t[2], tail); break;
    case RL_SDF: snprintf(name, cap, "fr::sdf_kernel<%s>", t[0] ? "true" : "false"); break;
    default: if (cap) name[0] = 0;
    }
}

}  // namespace fr

// raster_plan_selftest.cpp — the host rules of raster plans (csrc/fr_raster_plan.cpp) on the CPU: links fr_raster_plan.o
// and nothing else of the library.  Every case is a synthetic number table (no font, no GPU); it prints one line per case,
//   <case> <what the rule returned, field by field>
// (name/ lines: the kernel instances of a launch list as raster_launch_name prints them, each with its job count)
// which tests/test_raster_plan_tables.py compares with tests/golden/raster_plan_tables.json.  Job orders and tables of
// more than 16 entries are printed as an FNV-1a 64 hash.
#include "../csrc/fr_raster_plan.hpp"
#include "selftest.hpp"

#include <cstdio>
#include <string>
#include <vector>

using namespace selftest;

namespace {

// the glyph set of the plan cases: segment count, root bound, ray bound
struct G { uint32_t nseg, root, ray; };
const G GLYPHS[] = {{10, 20, 4}, {200, 200, 10}, {300, 400, 10}, {700, 900, 10}, {800, 900, 10}, {129, 100, 4}, {0, 0, 0}, {129, 2000, 4}};

const fr::RasterOpts DEFAULTS = {256u, 1u, 1u, 2048u, 1u, 4u, 4u, 32u};   // the context's defaults; both kernels: 4 waves

std::string hash(const void *v, size_t n, size_t size)
{
    uint64_t h = 0xcbf29ce484222325ull;
    for (size_t i = 0; i < n * size; ++i) h = (h ^ static_cast<const unsigned char *>(v)[i]) * 0x100000001b3ull;
    return fmt("#%zu:%016llx", n, (unsigned long long)h);
}

template <class T> std::string list(const T *v, size_t n)
{
    if (n > 16) return hash(v, n, sizeof(T));
    std::string s = "[";
    for (size_t i = 0; i < n; ++i) s += fmt(i ? ",%llu" : "%llu", (unsigned long long)v[i]);
    return s + "]";
}

fr_job job(uint32_t glyph, uint32_t w, uint32_t h, uint32_t out_x = 0, uint32_t out_y = 0)
{
    fr_job j{};
    j.glyph = glyph; j.min_x = 0; j.max_y = (int32_t)h; j.w = w; j.h = h; j.out_x = out_x; j.out_y = out_y; j.scale = 1.0f;
    return j;
}
void add(std::vector<fr_job> &v, uint32_t count, uint32_t glyph, uint32_t w, uint32_t h)
{
    for (uint32_t i = 0; i < count; ++i) v.push_back(job(glyph, w, h, (uint32_t)v.size() % 7u * 300u, (uint32_t)v.size() / 7u * 600u));
}

const char *FAMILY[] = {"prepare", "render", "cov4", "win1", "sdf"};

std::string launches(const fr::RasterPlan &p, const fr_raster_params &prm, uint32_t flags, fr::RasterOpts o, uint32_t max_seg)
{
    fr::RasterLaunchList L;
    fr::raster_launches(p, prm, flags, o, max_seg, L);
    std::string s = fmt("forked=%d join_at=%u", (int)L.forked, L.join_at);
    for (uint32_t i = 0; i < L.n; ++i) {
        const fr::RasterLaunch &e = L.l[i];
        s += fmt(" | %s mode=%d n=%d jobs=%u+%u strip_w=%u rec_cap=%u cell=%ux%u uniform=%d split=%u/%u largest=%d", FAMILY[e.family], e.mode,
                 e.samples, e.first, e.cnt, e.strip_w, e.rec_cap, e.bands, e.strips, (int)e.uniform, e.bands_per_wg, e.band_groups, (int)e.largest);
    }
    return s;
}

// the list's kernels as fr_plan_describe names them, in launch order (prepare launches have no name)
std::string names(const fr::RasterPlan &p, const fr_raster_params &prm, uint32_t flags, const fr::RasterOpts &o, uint32_t max_seg)
{
    fr::RasterLaunchList L;
    fr::raster_launches(p, prm, flags, o, max_seg, L);
    std::string s;
    for (uint32_t i = 0; i < L.n; ++i) {
        char name[96];
        fr::raster_launch_name(L.l[i], name, sizeof name);
        if (name[0]) s += fmt("%s%s x%u", s.empty() ? "" : "; ", name, L.l[i].cnt);
    }
    return s;
}

// the name of one launch: a hand-made plan of one job, on the fast kernels (a part of strips 16 << wlog with rec_cap
// record slots) or, rec_cap = 0, on the general one (strips of strip_w pixels)
std::string one_name(const fr_raster_params &prm, uint32_t flags, uint32_t kmax, uint32_t wlog, uint32_t rec_cap, uint32_t strip_w = 0,
                     bool uniform = false)
{
    fr::RasterOpts o = DEFAULTS;
    o.kmax = kmax;
    fr::RasterPlan p;
    p.n_jobs = p.pixels = 1;
    if (rec_cap) {
        p.n_fast = p.n_parts = 1;
        p.parts[0] = fr::RasterPart{0, 1, wlog, rec_cap, 1, 1, 1};
        p.fast_ns = fr::fast_rule(o, &prm).ns;
    } else {
        p.strip_w = strip_w; p.gen_bands = p.gen_strips = 1; p.uniform = uniform;
    }
    const std::string s = names(p, prm, flags, o, 0u);
    return s.substr(0, s.find(" x"));                                   // (FR_SDF_U8: the sign pass, not the distance kernel behind it)
}

struct Built {
    std::vector<uint8_t> cls;
    std::vector<uint32_t> order, jseg, large, jbits;
    std::vector<fr_job> sorted;
    fr::RasterPlan p;
};

// what fr_plan_create_ex asks for (single = false) and what fr_render_glyph_ex asks for its one job, whose glyph is `own`
void build(const std::vector<fr_job> &jobs, const fr_raster_params &prm, const fr::RasterOpts &o, Built &b, bool single = false,
           const G *own = nullptr, bool merge = false, bool uniform = false)
{
    std::vector<uint32_t> seg_start(1, 0u), root, ray;
    for (const G &g : GLYPHS) { seg_start.push_back(seg_start.back() + g.nseg); root.push_back(g.root); ray.push_back(g.ray); }
    if (single) { seg_start = {0u, own->nseg}; root = {own->root}; ray = {own->ray}; }
    const size_t n = jobs.size();
    b.cls.assign(n + 1, 0); b.order.assign(n + 1, 0); b.jseg.assign(2 * n + 1, 0); b.large.assign(n + 1, 0); b.jbits.assign(n + 1, 0);
    b.sorted.assign(n + 1, fr_job{});
    fr::RasterPlanIn in = fr::single_glyph_in(jobs.data(), seg_start.data(), root.data(), ray.data(), prm);
    if (single) { in.merge = merge; in.uniform = uniform; }              // (the two "asked" cases below)
    else { in.n_jobs = (uint32_t)n; in.sdf_fast = in.merge = in.uniform = true; }
    const fr::RasterTables t = {b.cls.data(), b.order.data(), b.sorted.data(), b.jseg.data(), b.large.data(), b.jbits.data()};
    fr::raster_plan_build(in, o, t, b.p);
    if (!b.p.too_many) fr::raster_plan_tables(in, t, b.p);
}

std::string plan_text(const Built &b)
{
    const fr::RasterPlan &p = b.p;
    std::string s = fmt("n_jobs=%u n_fast=%u fast_ns=%d strip_w=%u gen=%ux%u uniform=%d max=%ux%u pixels=%llu need=%llux%llu too_many=%d", p.n_jobs,
                        p.n_fast, p.fast_ns, p.strip_w, p.gen_bands, p.gen_strips, (int)p.uniform, p.max_w, p.max_h, (unsigned long long)p.pixels,
                        (unsigned long long)p.need_cols, (unsigned long long)p.need_rows, (int)p.too_many);
    s += " parts=";
    for (uint32_t i = 0; i < p.n_parts; ++i) {
        const fr::RasterPart &pt = p.parts[i];
        s += fmt("(%u+%u wlog=%u rec_cap=%u cell=%ux%u pixels=%llu)", pt.first, pt.cnt, pt.wlog, pt.rec_cap, pt.bands, pt.strips, (unsigned long long)pt.pixels);
    }
    if (p.too_many) return s;
    s += " order=" + list(b.order.data(), p.n_jobs) + " jobs=" + hash(b.sorted.data(), p.n_jobs, sizeof(fr_job));
    s += " jseg=" + list(b.jseg.data(), 2 * (size_t)p.n_jobs) + " large=" + list(b.large.data(), p.n_large);
    s += fmt(" bit_plane=%d bit_words=%llu", (int)p.bit_plane, (unsigned long long)p.bit_words);
    if (p.bit_plane) s += " jbits=" + list(b.jbits.data(), p.n_jobs);
    return s;
}

fr_raster_params params(int mode, int n) { return fr_raster_params{mode, n, FR_SAMPLE_CENTER}; }

// a plan: its tables, then its launch list under overlap 0 / 1 / 2
void plan_case(const char *name, const std::vector<fr_job> &jobs, const fr_raster_params &prm, uint32_t flags, fr::RasterOpts o)
{
    Built b;
    build(jobs, prm, o, b);
    printf("plan/%s %s\n", name, plan_text(b).c_str());
    if (b.p.too_many) return;
    for (uint32_t ov = 0; ov <= 2; ++ov) {
        o.overlap = ov;
        printf("launch/%s/overlap%u %s\n", name, ov, launches(b.p, prm, flags, o, 800u).c_str());
    }
    printf("name/plan/%s %s\n", name, names(b.p, prm, flags, o, 800u).c_str());
}

void single_case(const char *name, uint32_t w, uint32_t h, int mode, G g, fr::RasterOpts o = DEFAULTS, bool merge = false, bool uniform = false)
{
    Built b;
    const fr_raster_params prm = {mode, 1, FR_SAMPLE_CORNER};
    build({job(0, w, h)}, prm, o, b, true, &g, merge, uniform);
    printf("single/%s n_fast=%u n_large=%u bit_plane=%d %s\n", name, b.p.n_fast, b.p.n_large, (int)b.p.bit_plane,
           launches(b.p, prm, 0u, o, g.nseg).c_str());
    printf("name/single/%s %s\n", name, names(b.p, prm, 0u, o, g.nseg).c_str());
}

void bounds_case(const char *name, const std::vector<int16_t> &xy)         // xy: 6 numbers per segment (p0, p1, p2)
{
    std::vector<uint32_t> seg_p0;
    for (uint32_t s = 0; s < xy.size() / 6; ++s) seg_p0.push_back(3 * s);
    std::vector<std::pair<int32_t, int32_t>> ev;
    std::string s;
    for (size_t i = 0; i < xy.size(); ++i) s += fmt(i ? ",%d" : "%d", (int)xy[i]);
    printf("bounds/%s root=%u ray=%u segs=%s\n", name, fr::glyph_root_bound(xy.data(), seg_p0.data(), 0, (uint32_t)seg_p0.size()),
           fr::glyph_ray_bound(xy.data(), seg_p0.data(), 0, (uint32_t)seg_p0.size(), ev), s.c_str());
}

}  // namespace

int main()
{
    // ---- fast_rule: every mode x samples per axis, the strip width options, cov4 = 0
    for (int mode = FR_WINDING_I16; mode <= FR_SDF_U8; ++mode)
        for (int n : {1, 2, 3, 4, 8}) {
            const fr_raster_params prm = params(mode, n);
            const fr::FastRule r = fr::fast_rule(DEFAULTS, &prm);
            printf("fast_rule/mode%d/n%d ns=%d wlog_max=%u\n", mode, n, r.ns, r.wlog_max);
        }
    for (uint32_t px : {16u, 48u, 64u, 128u, 256u}) {
        fr::RasterOpts o = DEFAULTS;
        o.strip_px = px;
        const fr_raster_params prm = params(FR_COVERAGE_U8, 4);
        const fr::FastRule r = fr::fast_rule(o, &prm);
        printf("fast_rule/strip_px%u ns=%d wlog_max=%u\n", px, r.ns, r.wlog_max);
    }
    {
        fr::RasterOpts o = DEFAULTS;
        o.cov4 = 0;
        const fr_raster_params prm = params(FR_COVERAGE_U8, 4);
        const fr::FastRule r = fr::fast_rule(o, &prm);
        printf("fast_rule/cov4_0 ns=%d wlog_max=%u\n", r.ns, r.wlog_max);
    }
    // ---- fast_class on both sides of every threshold (ns = 4 unless said)
    {
        fr::FastRule R;
        R.ns = 4; R.wlog_max = 4;
        for (uint32_t w : {0u, 64u, 65u, 128u, 129u}) printf("fast_class/w%u %d\n", w, fr::fast_class(R, w, 30, 10, 20, 4));
        printf("fast_class/h0 %d\n", fr::fast_class(R, 30, 0, 10, 20, 4));
        for (uint32_t nsg : {256u, 257u, 384u, 385u, 768u, 769u}) printf("fast_class/nsg%u %d\n", nsg, fr::fast_class(R, 30, 30, nsg, 20, 4));
        for (uint32_t rb : {128u, 129u, 256u, 257u, 512u, 513u, 1024u, 1025u}) printf("fast_class/root%u %d\n", rb, fr::fast_class(R, 30, 30, 10, rb, 4));
        for (uint32_t ray : {16u, 17u}) printf("fast_class/ray%u %d\n", ray, fr::fast_class(R, 30, 30, 10, 20, ray));
        for (int ns : {1, 2, 4})
            for (uint32_t hs : {2048u, 2049u})
                printf("fast_class/ns%d/rows%u %d\n", ns, hs, fr::fast_class(fr::FastRule{ns, 4}, 30, (hs + (uint32_t)ns - 1u) / (uint32_t)ns, 10, 20, 4));
        for (uint32_t wl : {2u, 3u}) printf("fast_class/wlog_max%u/w300 %d\n", wl, fr::fast_class(fr::FastRule{4, wl}, 300, 30, 10, 20, 4));
        printf("fast_class/ns0 %d\n", fr::fast_class(fr::FastRule{0, 4}, 30, 30, 10, 20, 4));
    }
    // ---- merge_small_classes
    {
        struct M { const char *name; std::vector<std::pair<int, uint32_t>> classes; };
        const M cases[] = {{"63_into_64", {{0, 63}, {1, 64}}}, {"64_stays", {{0, 64}, {1, 64}}}, {"63_above_has_no_target", {{0, 64}, {1, 63}}},
                           {"chain", {{0, 10}, {1, 20}, {2, 100}}}, {"no_target", {{11, 5}}}, {"across_widths", {{1, 5}, {6, 70}}},
                           {"across_widths_not_fewer_slots", {{2, 5}, {5, 70}, {7, 3}}}};
        for (const M &m : cases) {
            uint32_t counts[fr::FAST_CLASSES] = {};
            std::vector<uint8_t> cls(1, 0);                              // (a general job among them)
            for (const auto &c : m.classes) { counts[c.first] = c.second; cls.push_back((uint8_t)(c.first + 1)); }
            fr::merge_small_classes(counts, cls.data(), (uint32_t)cls.size());
            printf("merge/%s counts=%s cls=%s\n", m.name, list(counts, fr::FAST_CLASSES).c_str(), list(cls.data(), cls.size()).c_str());
        }
    }
    // ---- split_bands
    for (uint32_t min_wgs : {0u, 1u, 2048u})
        for (uint32_t bands : {1u, 4u, 5u, 32u, 33u}) {
            const auto s = fr::split_bands(4, 3, bands, 2, min_wgs);
            printf("split_bands/min_wgs%u/bands%u %u %u\n", min_wgs, bands, s.first, s.second);
        }
    // ---- full plans, each with its launch list
    const fr_raster_params cov4 = params(FR_COVERAGE_U8, 4), sdf = params(FR_SDF_U8, 1);
    fr::RasterOpts general = DEFAULTS;
    general.cov4 = 0;
    plan_case("empty", {}, cov4, 0u, DEFAULTS);
    {
        std::vector<fr_job> j;
        add(j, 70, 0, 20, 20);
        plan_case("all_fast", j, cov4, 0u, DEFAULTS);
        plan_case("all_fast_gray", j, params(FR_GRAY_DEBUG, 1), 0u, DEFAULTS);
        plan_case("all_fast_winding_fill", j, params(FR_WINDING_I16, 1), FR_FILL_CONSISTENT, DEFAULTS);
    }
    {
        std::vector<fr_job> j;
        add(j, 5, 0, 64, 64);
        plan_case("all_general_uniform", j, cov4, 0u, general);
        add(j, 1, 0, 47, 45);
        plan_case("all_general_ragged", j, cov4, 0u, general);
        fr::RasterOpts unfused = general;
        unfused.fuse_prepare = 0;
        plan_case("all_general_unfused_fill", j, cov4, FR_FILL_CONSISTENT, unfused);
    }
    {
        std::vector<fr_job> j;
        add(j, 64, 0, 20, 20); add(j, 64, 0, 70, 20); add(j, 1, 4, 16, 520);
        plan_case("mixed", j, cov4, 0u, DEFAULTS);
        plan_case("mixed_sdf", j, sdf, 0u, DEFAULTS);
        plan_case("mixed_fill", j, cov4, FR_FILL_CONSISTENT, DEFAULTS);
        fr::RasterOpts few = DEFAULTS;
        few.min_wgs = 1;
        plan_case("mixed_min_wgs1", j, cov4, 0u, few);
        std::vector<fr_job> shuffled;
        for (size_t i = 0; i < j.size(); ++i) shuffled.push_back(j[(i * 50) % j.size()]);       // (50 and 129 are coprime)
        plan_case("mixed_shuffled", shuffled, cov4, 0u, DEFAULTS);
    }
    {
        std::vector<fr_job> j;
        add(j, 3, 0, 0, 10); add(j, 1, 0, 0, 0);
        plan_case("general_widest_w0", j, cov4, 0u, DEFAULTS);
    }
    {
        fr::RasterOpts o = DEFAULTS;
        o.strip_px = 48;
        std::vector<fr_job> j;
        add(j, 2, 0, 100, 30);
        plan_case("strip_px48", j, cov4, 0u, o);
        o.strip_px = 64;
        plan_case("strip_px64", j, cov4, 0u, o);
    }
    {
        std::vector<fr_job> j;
        add(j, 2, 4, 30, 30); add(j, 1, 7, 30, 30); add(j, 1, 4, 30, 30); add(j, 3, 5, 30, 30); add(j, 1, 0, 30, 30);
        plan_case("large_duplicates", j, cov4, 0u, DEFAULTS);
        j.clear();
        add(j, 3, 5, 30, 30); add(j, 1, 3, 30, 30);
        plan_case("large_among_fast_only", j, cov4, 0u, DEFAULTS);
    }
    {
        std::vector<fr_job> j;
        add(j, 1, 0, 256, 10); add(j, 1, 0, 257, 10); add(j, 1, 4, 30, 30); add(j, 1, 0, 1, 1);
        plan_case("sdf_bit_plane", j, sdf, 0u, DEFAULTS);
        j.clear();
        add(j, 2, 4, 30, 30);
        plan_case("sdf_all_general", j, sdf, 0u, DEFAULTS);
    }
    {
        // 65 535 x 65 535 general cells: 1024 bands x 256 strips each, 2^31 workgroups at 8192 of them
        std::vector<fr_job> j;
        add(j, 8191, 0, 65535, 65535);
        plan_case("wg_limit_below", j, params(FR_COVERAGE_U8, 1), 0u, general);
        add(j, 1, 0, 65535, 65535);
        plan_case("wg_limit_at", j, params(FR_COVERAGE_U8, 1), 0u, general);
    }
    for (uint32_t h : {7999u, 8000u}) {
        // two fast parts and a general job, 2^25 pixels with h = 8000: option overlap = 1 forks from there
        std::vector<fr_job> j;
        add(j, 64, 0, 64, 64); add(j, 64, 0, 128, 64); add(j, 1, 0, 4096, h);
        plan_case(h == 8000u ? "32mpixel_at" : "32mpixel_below", j, cov4, 0u, DEFAULTS);
    }
    // ---- the single-glyph call
    single_case("47x45", 47, 45, FR_GRAY_DEBUG, GLYPHS[0]);
    single_case("47x45_merge_asked", 47, 45, FR_GRAY_DEBUG, GLYPHS[0], DEFAULTS, true);         // (nothing to merge into: the same line)
    single_case("64x64", 64, 64, FR_GRAY_DEBUG, GLYPHS[0]);
    single_case("64x64_general", 64, 64, FR_GRAY_DEBUG, GLYPHS[0], general);
    single_case("64x64_general_as_a_plan_would", 64, 64, FR_GRAY_DEBUG, GLYPHS[0], general, false, true);   // (uniform: another instance)
    single_case("300wide", 300, 45, FR_WINDING_I16, GLYPHS[0]);
    single_case("300wide_general", 300, 45, FR_WINDING_I16, GLYPHS[0], general);
    single_case("sdf", 47, 45, FR_SDF_U8, GLYPHS[0]);
    single_case("sdf_129seg", 47, 45, FR_SDF_U8, GLYPHS[5]);
    single_case("129seg_general", 47, 45, FR_MASK_NONZERO, GLYPHS[7]);
    single_case("129seg_fast", 47, 45, FR_MASK_NONZERO, GLYPHS[5]);
    single_case("0seg", 47, 45, FR_GRAY_DEBUG, GLYPHS[6]);
    single_case("2049rows", 10, 2049, FR_GRAY_DEBUG, GLYPHS[0]);
    // ---- option kmax on both sides of 8, 16 and 32: the four record classes of cov4_kernel and the general kernel
    for (uint32_t kmax : {1u, 8u, 9u, 16u, 17u, 32u, 128u}) {
        for (uint32_t rec_cap : {128u, 256u, 512u, 1024u})
            printf("name/kmax%u/cov4_rec%u %s\n", kmax, rec_cap, one_name(cov4, 0u, kmax, 4u, rec_cap).c_str());
        printf("name/kmax%u/render %s\n", kmax, one_name(cov4, 0u, kmax, 0u, 0u, 256u).c_str());
    }
    // ---- every instance the rules can name: each value of each template argument, both fill rules
    for (uint32_t flags : {0u, (uint32_t)FR_FILL_CONSISTENT}) {
        std::string s;
        auto add = [&](const std::string &name) { if (s.find(name + ";") == std::string::npos) s += name + "; "; };   // (each once)
        for (int ns : {2, 4})
            for (uint32_t wlog : {2u, 3u, 4u})
                for (uint32_t rec_cap : {128u, 256u, 512u, 1024u})
                    for (uint32_t kmax : {8u, 16u, 32u}) add(one_name(params(FR_COVERAGE_U8, ns), flags, kmax, wlog, rec_cap));
        printf("name/sweep/cov4/fill%u %s\n", flags, s.c_str());
        s.clear();
        for (int mode : {FR_WINDING_I16, FR_GRAY_DEBUG, FR_MASK_NONZERO, FR_COVERAGE_U8, FR_SDF_U8})
            for (uint32_t wlog : {2u, 3u, 4u})
                for (uint32_t rec_cap : {128u, 256u, 512u, 1024u}) add(one_name(params(mode, 1), flags, 32u, wlog, rec_cap));
        printf("name/sweep/win1/fill%u %s\n", flags, s.c_str());
        s.clear();
        for (int mode : {FR_WINDING_I16, FR_GRAY_DEBUG, FR_MASK_NONZERO, FR_COVERAGE_U8, FR_SDF_U8})
            for (int n : {1, 2, 4})
                for (uint32_t kmax : {8u, 16u, 32u})
                    for (uint32_t strip_w : {48u, 64u, 128u, 256u})
                        for (bool uniform : {false, true})
                            if (n == 1 || mode == FR_COVERAGE_U8) add(one_name(params(mode, n), flags, kmax, 0u, 0u, strip_w, uniform));
        printf("name/sweep/render/fill%u %s\n", flags, s.c_str());
    }
    // ---- root and ray bounds of hand-written segments
    bounds_case("line", {0, 0, 5, 5, 10, 10});
    bounds_case("horizontal", {0, 7, 5, 7, 10, 7});
    bounds_case("horizontal_bulge", {0, 7, 5, 12, 10, 7});
    bounds_case("overshoot_above", {0, 0, 5, 30, 10, 10});
    bounds_case("overshoot_below", {0, 0, 5, -31, 10, 10});
    bounds_case("monotone_curve", {0, 0, 0, 2, 10, 10});
    bounds_case("control_at_end", {0, 0, 5, 10, 10, 10});
    bounds_case("square", {0, 0, 5, 0, 10, 0, 10, 0, 10, 5, 10, 10, 10, 10, 5, 10, 0, 10, 0, 10, 0, 5, 0, 0});
    bounds_case("stack", {0, 0, 5, 20, 10, 0, 0, 5, 5, 25, 10, 5, 0, 10, 5, -9, 10, 12, 3, -4, 5, 8, 7, -4});
    bounds_case("empty", {});
    return 0;
}

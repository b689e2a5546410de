// host_rules_selftest.cpp — the host arithmetic of the C ABI (csrc/fr_host_rules.cpp) on the CPU: links fr_host_rules.o and
// nothing else of the library.  No font, no GPU; it prints one line per case,
//   <case> rc=<code> <what came back, field by field>        or        <case> rc=<code> err=<the message left>
// which tests/test_host_rules.py compares with tests/golden/host_rules.json.  Tables are printed as an FNV-1a 64 hash of
// their bytes.  tools/mint_host_rules.py makes the same calls on a built library through ctypes: the case tables
// here and there are the same, line for line.
#include "../csrc/fr_host_rules.hpp"
#include "selftest.hpp"

#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

using namespace selftest;

namespace {

std::string hash(const void *v, size_t bytes)
{
    uint64_t h = 0xcbf29ce484222325ull;
    for (size_t i = 0; i < bytes; ++i) h = (h ^ static_cast<const unsigned char *>(v)[i]) * 0x100000001b3ull;
    return fmt("#%zu:%016llx", bytes, (unsigned long long)h);
}

void line(const std::string &name, int rc, const std::string &fields)
{
    printf("%s rc=%d %s\n", name.c_str(), rc, rc ? fmt("err=%s", last_error()).c_str() : fields.c_str());
}

std::string job_text(const fr_job &j)
{
    uint32_t bits;
    memcpy(&bits, &j.scale, 4);
    return fmt("%u,%d,%d,%u,%u,%u,%u,%08x", j.glyph, j.min_x, j.max_y, j.w, j.h, j.out_x, j.out_y, bits);
}

// glyph i of the layout cases: a box that changes in every field, and the per-glyph units per em
void box_of(uint32_t i, int16_t b[4])
{
    b[0] = (int16_t)-(int)(i * 37u % 200u); b[1] = (int16_t)-(int)(i * 91u % 300u);
    b[2] = (int16_t)(100u + i * 53u % 900u); b[3] = (int16_t)(200u + i * 29u % 1200u);
}
uint16_t upm_of(uint32_t i) { return (uint16_t)(1000u + (i % 3u) * 512u); }

struct Glyphs {
    std::vector<int16_t> boxes;
    std::vector<uint16_t> upm;
};
// upm1 != 0: one value for all; else one per glyph.  tall: every box is (0, 0, 10, 32765)
Glyphs glyphs(uint32_t n, uint16_t upm1, bool tall = false)
{
    Glyphs g;
    g.boxes.resize(4 * (size_t)n);
    for (uint32_t i = 0; i < n; ++i) {
        if (tall) { const int16_t b[4] = {0, 0, 10, 32765}; memcpy(&g.boxes[4 * (size_t)i], b, 8); }
        else box_of(i, &g.boxes[4 * (size_t)i]);
    }
    if (upm1) g.upm.assign(1, upm1);
    else for (uint32_t i = 0; i < n; ++i) g.upm.push_back(upm_of(i));
    return g;
}

// ---- fr_render_glyph_dims ---------------------------------------------------------------------------------------------
struct DimsCase { const char *name; int16_t box[4]; uint16_t upm, size; };
const DimsCase DIMS[] = {
    {"fraction", {-3, -7, 1001, 1503}, 2048, 64},
    {"tiny", {10, 20, 30, 40}, 65535, 1},
    {"point", {0, 0, 0, 0}, 1, 65535},
    {"negative", {-900, -800, -100, -50}, 1000, 333},
    {"w32767", {0, 0, 32766, 10}, 1, 1},
    {"w32768", {0, 0, 32767, 10}, 1, 1},
    {"h32767", {0, -32766, 10, 0}, 1, 1},
    {"h32768", {0, -32767, 10, 0}, 1, 1},
    {"min-32768", {-32768, -5, -2, 5}, 1, 1},
    {"min-32768wide", {-32768, -5, -1, 5}, 1, 1},
    {"hi32767", {32760, 0, 32767, 10}, 1, 1},
    {"scaled-hi-in", {0, 0, 16383, 100}, 1, 2},
    {"scaled-hi-out", {0, 0, 16384, 100}, 1, 2},
    {"scaled-hi-y-out", {0, 0, 100, 16384}, 1, 2},
    {"scaled-lo-in", {-16384, 0, -16000, 10}, 1, 2},
    {"scaled-lo-out", {-16385, 0, -16000, 10}, 1, 2},
    {"scaled-lo-y-out", {0, -16385, 10, -16000}, 1, 2},
    {"upm0", {0, 0, 10, 10}, 0, 10},
    {"size0", {0, 0, 10, 10}, 10, 0},
};

void dims_cases()
{
    for (const DimsCase &c : DIMS) {
        int16_t mn[2] = {0, 0}, mx[2] = {0, 0};
        uint16_t w = 0, h = 0;
        float scale = 0.f;
        const int rc = fr_render_glyph_dims(c.box, c.upm, c.size, mn, mx, &w, &h, &scale);
        uint32_t bits;
        memcpy(&bits, &scale, 4);
        line(fmt("dims/%s", c.name), rc, fmt("min=%d,%d max=%d,%d size=%ux%u scale=%08x", mn[0], mn[1], mx[0], mx[1], w, h, bits));
    }
    int16_t mn[2], mx[2];
    uint16_t w, h;
    const int16_t box[4] = {0, 0, 10, 10};
    line("dims/null-box", fr_render_glyph_dims(nullptr, 10, 10, mn, mx, &w, &h, nullptr), "");
    line("dims/null-width", fr_render_glyph_dims(box, 10, 10, mn, mx, nullptr, &h, nullptr), "");
    const int rc = fr_render_glyph_dims(box, 10, 10, mn, mx, &w, &h, nullptr);
    line("dims/without-scale", rc, fmt("size=%ux%u", w, h));
}

// ---- fr_atlas_layout ----------------------------------------------------------------------------------------------------
// boxes / jobs / upm: 0 passes NULL
struct CellCase { const char *name; uint32_t n, first; uint16_t upm1; uint32_t n_upm; uint16_t size; uint32_t cell, cols, rows_per_page; int boxes, jobs, upm; };
const CellCase CELLS[] = {
    {"one-page", 10, 5, 2048, 1, 64, 64, 4, 0, 1, 1, 1},
    {"pages-upm-per-glyph", 23, 0, 0, 23, 48, 32, 5, 2, 1, 1, 1},
    {"page-exact", 12, 100, 1000, 1, 20, 16, 3, 2, 1, 1, 1},
    {"one-glyph-upm-both", 1, 7, 0, 1, 64, 128, 1, 1, 1, 1, 1},
    {"empty", 0, 0, 1000, 1, 64, 64, 4, 0, 0, 0, 1},
    {"null-boxes", 3, 0, 1000, 1, 64, 64, 4, 0, 0, 1, 1},
    {"null-jobs", 3, 0, 1000, 1, 64, 64, 4, 0, 1, 0, 1},
    {"null-upm", 3, 0, 1000, 1, 64, 64, 4, 0, 1, 1, 0},
    {"n-upm-2-of-5", 5, 0, 0, 2, 64, 64, 4, 0, 1, 1, 1},
    {"cell-0", 3, 0, 1000, 1, 64, 0, 4, 0, 1, 1, 1},
    {"cols-0", 3, 0, 1000, 1, 64, 64, 0, 0, 1, 1, 1},
    {"size-0", 3, 0, 1000, 1, 0, 64, 4, 0, 1, 1, 1},
    {"too-wide", 3, 0, 1000, 1, 64, 65536, 65536, 0, 1, 1, 1},
    {"widest", 3, 0, 1000, 1, 64, 65535, 65537, 0, 1, 1, 1},
    {"too-tall", 3, 0, 1000, 1, 64, 0x80000000u, 1, 0, 1, 1, 1},
    {"tallest", 2, 0, 1000, 1, 64, 0x80000000u, 1, 0, 1, 1, 1},
    {"tall-paged", 5, 0, 1000, 1, 64, 0x80000000u, 1, 2, 1, 1, 1},
};

void cell_cases()
{
    for (const CellCase &c : CELLS) {
        Glyphs g = glyphs(c.n, c.upm1);
        if (c.upm1 == 0 && c.n_upm < c.n) g.upm.resize(c.n_upm);
        std::vector<fr_job> jobs(c.n);
        std::vector<uint32_t> page(c.n);
        uint32_t n_pages = 0;
        const int rc = fr_atlas_layout(c.boxes ? g.boxes.data() : nullptr, c.n, c.first, c.upm ? g.upm.data() : nullptr, c.n_upm, c.size, c.cell,
                                       c.cols, c.rows_per_page, c.jobs ? jobs.data() : nullptr, page.data(), &n_pages);
        line(fmt("cells/%s", c.name), rc,
             fmt("n=%u jobs=%s last=%s page_of=%s pages=%u", c.n, hash(jobs.data(), c.n * sizeof(fr_job)).c_str(),
                 c.n ? job_text(jobs[c.n - 1]).c_str() : "-", hash(page.data(), c.n * 4u).c_str(), n_pages));
    }
    {   // units per em of 0 among the per-glyph values; and the optional outputs left out
        Glyphs g = glyphs(4, 0);
        g.upm[2] = 0;
        std::vector<fr_job> jobs(4);
        line("cells/upm-0-at-2", fr_atlas_layout(g.boxes.data(), 4, 0, g.upm.data(), 4, 64, 64, 4, 0, jobs.data(), nullptr, nullptr), "");
        g.upm[2] = 1000;
        const int rc = fr_atlas_layout(g.boxes.data(), 4, 0, g.upm.data(), 4, 64, 64, 4, 0, jobs.data(), nullptr, nullptr);
        line("cells/no-page-outputs", rc, fmt("jobs=%s", hash(jobs.data(), 4 * sizeof(fr_job)).c_str()));
    }
}

// ---- fr_atlas_layout_glyph_dims -------------------------------------------------------------------------------------------
struct ShelfCase { const char *name; uint32_t n, first; uint16_t upm1; uint32_t n_upm; uint16_t size; uint32_t atlas_w, align; int boxes, jobs, upm, tall; };
const ShelfCase SHELVES[] = {
    {"wrap", 20, 0, 1000, 1, 100, 300, 1, 1, 1, 1, 0},
    {"align-16-upm-per-glyph", 20, 3, 0, 20, 64, 256, 16, 1, 1, 1, 0},
    {"align-0", 5, 0, 2048, 1, 200, 4096, 0, 1, 1, 1, 0},
    {"align-7-tight", 9, 0, 1000, 1, 50, 60, 7, 1, 1, 1, 0},
    {"one-glyph-upm-both", 1, 9, 0, 1, 64, 64, 1, 1, 1, 1, 0},
    {"empty", 0, 0, 1000, 1, 64, 64, 1, 0, 0, 1, 0},
    {"null-boxes", 3, 0, 1000, 1, 64, 640, 1, 0, 1, 1, 0},
    {"null-jobs", 3, 0, 1000, 1, 64, 640, 1, 1, 0, 1, 0},
    {"null-upm", 3, 0, 1000, 1, 64, 640, 1, 1, 1, 0, 0},
    {"n-upm-2-of-5", 5, 0, 0, 2, 64, 640, 1, 1, 1, 1, 0},
    {"atlas-w-0", 3, 0, 1000, 1, 64, 0, 1, 1, 1, 1, 0},
    {"size-0", 3, 0, 1000, 1, 0, 640, 1, 1, 1, 1, 0},
    {"glyph-too-wide", 3, 0, 1000, 1, 64, 4, 1, 1, 1, 1, 0},
    {"box-leaves-i16", 3, 0, 1, 1, 65535, 640, 1, 1, 1, 1, 0},
    {"tallest", 131080, 0, 1, 1, 1, 11, 1, 1, 1, 1, 1},
    {"too-tall", 131081, 0, 1, 1, 1, 11, 1, 1, 1, 1, 1},
};

void shelf_cases()
{
    for (const ShelfCase &c : SHELVES) {
        Glyphs g = glyphs(c.n, c.upm1, c.tall != 0);
        if (c.upm1 == 0 && c.n_upm < c.n) g.upm.resize(c.n_upm);
        std::vector<fr_job> jobs(c.n);
        uint32_t atlas_h = 0;
        const int rc = fr_atlas_layout_glyph_dims(c.boxes ? g.boxes.data() : nullptr, c.n, c.first, c.upm ? g.upm.data() : nullptr, c.n_upm, c.size,
                                                  c.atlas_w, c.align, c.jobs ? jobs.data() : nullptr, &atlas_h);
        line(fmt("shelves/%s", c.name), rc,
             fmt("n=%u jobs=%s last=%s atlas_h=%u", c.n, hash(jobs.data(), c.n * sizeof(fr_job)).c_str(),
                 c.n ? job_text(jobs[c.n - 1]).c_str() : "-", atlas_h));
    }
    {
        Glyphs g = glyphs(4, 0);
        g.upm[2] = 0;
        std::vector<fr_job> jobs(4);
        line("shelves/upm-0-at-2", fr_atlas_layout_glyph_dims(g.boxes.data(), 4, 0, g.upm.data(), 4, 64, 640, 1, jobs.data(), nullptr), "");
        g.upm[2] = 1000;
        const int rc = fr_atlas_layout_glyph_dims(g.boxes.data(), 4, 0, g.upm.data(), 4, 64, 640, 1, jobs.data(), nullptr);
        line("shelves/no-height-output", rc, fmt("jobs=%s", hash(jobs.data(), 4 * sizeof(fr_job)).c_str()));
    }
}

// ---- the sRGB conversions and the unpremultiply ---------------------------------------------------------------------------
void colour_cases()
{
    std::vector<uint8_t> codes(256), back(256);
    std::vector<uint16_t> lin(256);
    for (int i = 0; i < 256; ++i) codes[i] = (uint8_t)i;
    int rc = fr_srgb_decode(codes.data(), 256, lin.data());
    line("srgb/decode-all-codes", rc, fmt("first=%u last=%u table=%s", lin[0], lin[255], hash(lin.data(), 512).c_str()));
    rc = fr_srgb_encode(lin.data(), 256, back.data());
    line("srgb/encode-decoded", rc, fmt("same=%d", (int)(back == codes)));
    std::vector<uint16_t> all(65536);
    std::vector<uint8_t> enc(65536);
    for (uint32_t i = 0; i < 65536u; ++i) all[i] = (uint16_t)i;
    rc = fr_srgb_encode(all.data(), 65536, enc.data());
    line("srgb/encode-all-values", rc, fmt("first=%u last=%u table=%s", enc[0], enc[65535], hash(enc.data(), 65536).c_str()));
    line("srgb/decode-null", fr_srgb_decode(nullptr, 1, lin.data()), "");
    line("srgb/encode-null", fr_srgb_encode(all.data(), 1, nullptr), "");
    line("srgb/decode-nothing", fr_srgb_decode(nullptr, 0, nullptr), "ok");
    line("srgb/encode-nothing", fr_srgb_encode(nullptr, 0, nullptr), "ok");
    // every (channel, alpha) pair, channel values above alpha (not premultiplied: they saturate) included: pixel
    // 256 * a + c is (c, 255 - c, c ^ 0x55, a)
    for (int srgb = 0; srgb < 2; ++srgb) {
        std::vector<uint8_t> px(4u * 65536u);
        for (uint32_t a = 0; a < 256u; ++a)
            for (uint32_t c = 0; c < 256u; ++c) {
                uint8_t *p = &px[4u * (256u * a + c)];
                p[0] = (uint8_t)c; p[1] = (uint8_t)(255u - c); p[2] = (uint8_t)(c ^ 0x55u); p[3] = (uint8_t)a;
            }
        rc = fr_rgba_unpremultiply(px.data(), 65536, srgb);
        line(fmt("unpremultiply/%s-all-pairs", srgb ? "srgb" : "linear"), rc, fmt("image=%s", hash(px.data(), px.size()).c_str()));
    }
    line("unpremultiply/null", fr_rgba_unpremultiply(nullptr, 1, 0), "");
    line("unpremultiply/nothing", fr_rgba_unpremultiply(nullptr, 0, 1), "ok");
}

// ---- the argument checks: each limit on both sides ------------------------------------------------------------------------
struct KCase { const char *name; uint32_t K; int32_t x0, y0; uint32_t w, h; };
const int32_t M = 1 << 20;
const KCase KS[] = {
    {"K-0", 0, 0, 0, 4, 4}, {"K-1", 1, 0, 0, 4, 4}, {"K-8", 8, 0, 0, 4, 4}, {"K-9", 9, 0, 0, 4, 4},
    {"w-max", 1, -M, 0, 1u << 20, 4}, {"w-over", 1, -M, 0, (1u << 20) + 1u, 4},
    {"h-max", 1, 0, M, 4, 1u << 20}, {"h-over", 1, 0, M, 4, (1u << 20) + 1u},
    {"x0-min", 1, -M, 0, 4, 4}, {"x0-under", 1, -M - 1, 0, 4, 4},
    {"x1-max", 1, M - 4, 0, 4, 4}, {"x1-over", 1, M - 3, 0, 4, 4},
    {"y0-max", 1, 0, M, 4, 4}, {"y0-over", 1, 0, M + 1, 4, 4},
    {"y1-min", 1, 0, -M + 4, 4, 4}, {"y1-under", 1, 0, -M + 3, 4, 4},
    {"empty", 3, 0, 0, 0, 0},
};

fr_job job(uint32_t glyph, int32_t min_x, int32_t max_y, uint32_t w, uint32_t h, float scale)
{
    fr_job j{};
    j.glyph = glyph; j.min_x = min_x; j.max_y = max_y; j.w = w; j.h = h; j.scale = scale;
    return j;
}

void check_cases()
{
    for (const KCase &c : KS) line(fmt("check_k/%s", c.name), fr::check_k(c.K, c.x0, c.y0, c.w, c.h), "ok");

    line("check_params/null", fr::check_params(nullptr), "");
    for (int mode = -1; mode <= 5; ++mode)
        for (int n : {0, 1, 2, 3, 4, 8})
            for (int phase : {-1, 0, 1, 2}) {
                if (phase != 0 && (n != 1 || (mode != 0 && mode != 3))) continue;      // the phase: with a valid mode and n only
                const fr_raster_params p = {mode, n, phase, 0};
                line(fmt("check_params/mode%d-n%d-phase%d", mode, n, phase), fr::check_params(&p), "ok");
            }

    const uint32_t text = FR_TEXT_SRGB | FR_TEXT_BGRA | FR_TEXT_LOAD | FR_TEXT_OVER;
    const struct { const char *name; uint32_t flags, also; } FLAGS[] = {
        {"none", 0u, 0u}, {"fill", FR_FILL_CONSISTENT, 0u}, {"bit1", 2u, 0u}, {"srgb-plain", FR_TEXT_SRGB, 0u},
        {"text-all", FR_FILL_CONSISTENT | text, text}, {"cache-not-taken", FR_TEXT_CACHE, text}, {"cache", FR_TEXT_CACHE, text | FR_TEXT_CACHE},
        {"bit6", 64u, text | FR_TEXT_CACHE}, {"bit9", 512u, text | FR_TEXT_CACHE}, {"top", 0x80000000u, text | FR_TEXT_CACHE},
        {"several", 0x80000002u | FR_FILL_CONSISTENT, 0u},
    };
    for (const auto &c : FLAGS) line(fmt("check_flags/%s", c.name), fr::check_flags(c.flags, c.also), "ok");

    const int32_t E = 1 << 22;
    const float lo = 9.5367431640625e-07f, hi = 1048576.0f;       // 2^-20, 2^20
    float below, above, inf, nan;
    const uint32_t bb = 0x357fffffu, ab = 0x49800001u, ib = 0x7f800000u, nb = 0x7fc00000u;
    memcpy(&below, &bb, 4); memcpy(&above, &ab, 4); memcpy(&inf, &ib, 4); memcpy(&nan, &nb, 4);
    const struct { const char *name; fr_job jb; } JOBS[] = {
        {"plain", job(0, 0, 64, 64, 64, 1.0f)},
        {"glyph-last", job(9, 0, 64, 64, 64, 1.0f)}, {"glyph-over", job(10, 0, 64, 64, 64, 1.0f)},
        {"scale-0", job(0, 0, 64, 64, 64, 0.0f)}, {"scale-negative", job(0, 0, 64, 64, 64, -1.0f)},
        {"scale-inf", job(0, 0, 64, 64, 64, inf)}, {"scale-nan", job(0, 0, 64, 64, 64, nan)},
        {"scale-min", job(0, 0, 64, 64, 64, lo)}, {"scale-under", job(0, 0, 64, 64, 64, below)},
        {"scale-max", job(0, 0, 64, 64, 64, hi)}, {"scale-over", job(0, 0, 64, 64, 64, above)},
        {"w-max", job(0, 0, 64, 65535, 64, 1.0f)}, {"w-over", job(0, 0, 64, 65536, 64, 1.0f)},
        {"h-max", job(0, 0, 64, 64, 65535, 1.0f)}, {"h-over", job(0, 0, 64, 64, 65536, 1.0f)},
        {"min-x-min", job(0, -E, 64, 64, 64, 1.0f)}, {"min-x-under", job(0, -E - 1, 64, 64, 64, 1.0f)},
        {"right-max", job(0, E - 64, 64, 64, 64, 1.0f)}, {"right-over", job(0, E - 63, 64, 64, 64, 1.0f)},
        {"max-y-max", job(0, 0, E, 64, 64, 1.0f)}, {"max-y-over", job(0, 0, E + 1, 64, 64, 1.0f)},
        {"bottom-min", job(0, 0, -E + 64, 64, 64, 1.0f)}, {"bottom-under", job(0, 0, -E + 63, 64, 64, 1.0f)},
        {"empty-cell", job(0, 0, 0, 0, 0, 1.0f)},
    };
    for (const auto &c : JOBS) line(fmt("check_job/%s", c.name), fr::check_job(10, c.jb, 3), "ok");
    line("scale_in_range", 0, fmt("min=%d under=%d max=%d over=%d nan=%d", (int)fr::scale_in_range(lo), (int)fr::scale_in_range(below), (int)fr::scale_in_range(hi),
                                  (int)fr::scale_in_range(above), (int)fr::scale_in_range(nan)));
}

// ---- fr_render_glyph's arena ----------------------------------------------------------------------------------------------
void arena_cases()
{
    const struct { uint64_t np; uint32_t ns; size_t rec, img; } A[] = {
        {0, 0, 32, 1}, {3, 1, 32, 47 * 45}, {37, 18, 32, 2 * 47 * 45}, {401, 200, 32, 300 * 300}, {2048, 1024, 48, 16}, {5, 2, 32, 0},
    };
    for (const auto &c : A) {
        const fr::GlyphArena a = fr::glyph_arena(c.np, c.ns, c.rec, c.img);
        line(fmt("arena/np%llu-ns%u-rec%zu-img%zu", (unsigned long long)c.np, c.ns, c.rec, c.img), 0,
             fmt("pts=%zu p0=%zu spts=%zu gseg=%zu job=%zu jseg=%zu large=%zu up=%zu cnt=%zu recs=%zu out=%zu total=%zu", a.pts, a.p0, a.spts, a.gseg,
                 a.job, a.jseg, a.large, a.up, a.cnt, a.recs, a.out, a.total));
    }
}

}  // namespace

int main()
{
    dims_cases();
    cell_cases();
    shelf_cases();
    colour_cases();
    check_cases();
    arena_cases();
    return 0;
}

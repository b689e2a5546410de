// fr_text_plan.cpp — from the placements and runs of a text plan to its host tables (fr_text_plan.hpp; include/fr_raster.h
// and DESIGN.md section 5 define what they mean).  Plain integer and binary32 host arithmetic, compiled by g++ with
// -ffp-contract=off: no HIP.  The three placement forms share one text, text_plan_tables; what differs per placement is
// four small pieces, overloaded on the form and written next to each other below: pen_of (how the fields are read),
// resolve (the form's own checks, and what the build keeps of them: the affine inverse), cell_of (the cell in pixels about the pen) and
// finish (the tail of the instance record).  The order of the checks fixes which error a caller sees: it is part of
// the ABI's behaviour and host/text_plan_selftest.cpp pins it.  A second builder, text_cache_tables, adds the tables of an
// FR_TEXT_CACHE or FR_TEXT_CACHE_AFFINE plan from the same pieces (host/text_cache_selftest.cpp,
// host/text_cache_affine_selftest.cpp).  At the end: from a plan's flags and counts to the
// launches of one render and their kernel names (text_plan_of, text_launches, text_launch_name).
#include "fr_text_plan.hpp"
#include "fr_srgb.hpp"

#include <algorithm>
#include <array>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>
#include <type_traits>
#include <utility>

namespace fr {
int set_error(int code, const char *fmt, ...);          // fr_api.hip (the self-test has its own)

namespace {

constexpr int64_t LIM = (int64_t)1 << 22;               // pens and cells stay within +-2^22 pixels

// the 4 bytes R G B A as one little-endian word, R in the low byte (fr_text_tables.hpp: TextInst::rgba, TextRun::clear); bgra
// (FR_TEXT_BGRA): B in the low byte, so that the kernels, which treat R and B alike, write B G R A
static uint32_t rgba_word(const uint8_t *c, bool bgra)
{
    return (uint32_t)c[bgra ? 2 : 0] | (uint32_t)c[1] << 8 | (uint32_t)c[bgra ? 0 : 2] << 16 | (uint32_t)c[3] << 24;
}

// an sRGB text plan's linear colour of a packed word (fr_text_tables.hpp: TextInst::pad, TextRun::pad; fr_srgb.hpp)
static void linear_words(uint32_t w, uint32_t pad[2])
{
    pad[0] = (uint32_t)fr::SRGB_D[w & 0xffu] | (uint32_t)fr::SRGB_D[(w >> 8) & 0xffu] << 16;
    pad[1] = fr::SRGB_D[(w >> 16) & 0xffu];
}

// D = xx*yy - xy*yx of an fr_glyph_place_affine in binary64: two rounded products and one rounded difference.  Not
// inlined and compiled without contraction, so that no fused multiply-add can take the place of a product's rounding.
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
__attribute__((noinline)) static double affine_det(double xx, double xy, double yx, double yy)
{
    volatile double a = xx * yy, b = xy * yx;
    return a - b;
}

// the inverse of an fr_glyph_place_affine's matrix (include/fr_raster.h) -> q[4]; FR_OK, or the code the header names
static int affine_inverse(const float m[4], float q[4])
{
    for (int i = 0; i < 4; ++i)
        if (!std::isfinite(m[i])) return FR_E_INVALID;
    const double D = affine_det((double)m[0], (double)m[1], (double)m[2], (double)m[3]);
    if (D == 0.0) return FR_E_INVALID;
    for (int i = 0; i < 4; ++i)
        if (std::fabs(m[i]) > 1048576.0f) return FR_E_UNSUPPORTED;
    q[0] = (float)((double)m[3] / D);
    q[1] = (float)(-(double)m[1] / D);
    q[2] = (float)(-(double)m[2] / D);
    q[3] = (float)((double)m[0] / D);
    for (int i = 0; i < 4; ++i)
        if (!(std::fabs(q[i]) <= 1048576.0f)) return FR_E_UNSUPPORTED;
    return FR_OK;
}

// ---- the placement forms ----------------------------------------------------------------------------------------------
struct Pen { uint32_t glyph; int32_t x64; int64_t y64; };   // y in 64 bits: 64 * pen_y of an fr_glyph_place need not fit 32
struct Cell { int64_t mnx, mxx, mny, mxy; };                // pixels about the pen, y up: columns mnx .. mxx, rows -mxy .. -mny
struct Inverse { float q[4]; };                             // of an fr_glyph_place_affine's matrix: resolve leaves inv[k] for finish

// the plain form is the _ex form with pen_y64 = 64 * pen_y, scale 0 and slant 0
Pen pen_of(const fr_glyph_place &p) { return Pen{p.glyph, p.pen_x64, (int64_t)64 * p.pen_y}; }
Pen pen_of(const fr_glyph_place_ex &p) { return Pen{p.glyph, p.pen_x64, p.pen_y64}; }
Pen pen_of(const fr_glyph_place_affine &p) { return Pen{p.glyph, p.pen_x64, p.pen_y64}; }

int resolve(const fr_glyph_place &, uint32_t, std::vector<Inverse> &) { return FR_OK; }
int resolve(const fr_glyph_place_ex &p, uint32_t k, std::vector<Inverse> &)
{
    const float ps = p.scale, sl = p.slant;
    if (!(ps >= 0.0f) || !std::isfinite(ps)) return set_error(FR_E_INVALID, "place %u: scale must be 0, or finite and > 0", k);
    if (ps != 0.0f && (ps < 9.5367431640625e-07f || ps > 1048576.0f))
        return set_error(FR_E_UNSUPPORTED, "place %u: scale outside [2^-20, 2^20]", k);
    if (!std::isfinite(sl)) return set_error(FR_E_INVALID, "place %u: slant must be finite", k);
    if (std::fabs(sl) > 4.0f) return set_error(FR_E_UNSUPPORTED, "place %u: |slant| above 4", k);
    return FR_OK;
}
int resolve(const fr_glyph_place_affine &p, uint32_t k, std::vector<Inverse> &inv)
{
    const int frc = affine_inverse(p.m, inv[k].q);
    if (frc == FR_E_INVALID) return set_error(frc, "place %u: matrix not finite or singular", k);
    if (frc != FR_OK) return set_error(frc, "place %u: matrix or its inverse beyond 2^20", k);
    return FR_OK;
}

float scale_of(const fr_glyph_place_ex &p, float run_scale) { return p.scale != 0.0f ? p.scale : run_scale; }

// render_glyph.zig:13-17 in binary32, as fr_render_glyph_dims / fr_atlas_layout, of the box b sheared by the slant k:
// lo = min(x_min + k*y_min, x_min + k*y_max), hi likewise, one rounding per operation; with k = 0 lo = x_min and hi = x_max
Cell sheared_cell(const int16_t *b, float s, float k)
{
    const float ky0 = k * (float)b[1], ky1 = k * (float)b[3];
    const float lo = std::min((float)b[0] + ky0, (float)b[0] + ky1);
    const float hi = std::max((float)b[2] + ky0, (float)b[2] + ky1);
    return Cell{(int64_t)std::floor(lo * s), (int64_t)std::ceil(hi * s), (int64_t)std::floor((float)b[1] * s), (int64_t)std::ceil((float)b[3] * s)};
}
Cell cell_of(const fr_glyph_place &, const int16_t *b, float run_scale) { return sheared_cell(b, run_scale, 0.0f); }
Cell cell_of(const fr_glyph_place_ex &p, const int16_t *b, float run_scale) { return sheared_cell(b, scale_of(p, run_scale), p.slant); }
// the box's four corners through the matrix, one rounding per operation (the products are stored before they are added:
// nothing here may be contracted)
Cell cell_of(const fr_glyph_place_affine &p, const int16_t *b, float)
{
    const float *m = p.m;
    float ulo = 0, uhi = 0, vlo = 0, vhi = 0;
    for (int c = 0; c < 4; ++c) {
        const float x = (float)b[(c & 1) ? 2 : 0], y = (float)b[(c & 2) ? 3 : 1];
        volatile float ux = m[0] * x, uy = m[1] * y, vx = m[2] * x, vy = m[3] * y;
        const float u = ux + uy, v = vx + vy;
        ulo = c ? std::min(ulo, u) : u; uhi = c ? std::max(uhi, u) : u;
        vlo = c ? std::min(vlo, v) : v; vhi = c ? std::max(vhi, v) : v;
    }
    return Cell{(int64_t)std::floor(ulo), (int64_t)std::ceil(uhi), (int64_t)std::floor(vlo), (int64_t)std::ceil(vhi)};
}

// what an instance record holds after the twelve common fields
void finish(TextInst &, const fr_glyph_place &, const std::vector<Inverse> &, uint32_t, uint32_t, float) {}
void finish(TextInstEx &i, const fr_glyph_place_ex &p, const std::vector<Inverse> &, uint32_t, uint32_t fy64, float run_scale)
{
    i.fy64 = fy64; i.scale = scale_of(p, run_scale); i.slant = p.slant;
}
void finish(TextInstAffine &i, const fr_glyph_place_affine &, const std::vector<Inverse> &inv, uint32_t k, uint32_t fy64, float)
{
    const float *q = inv[k].q;
    i.fy64 = fy64; i.q00 = q[0]; i.q01 = q[1]; i.q10 = q[2]; i.q11 = q[3];
}

}  // namespace

// ---- the one text over them -------------------------------------------------------------------------------------------
template <class PLACE>
int text_plan_tables(const TextPlanIn &in, const PLACE *places, TextPlanTables<PLACE> &out)
{
    using INST = typename TextInstOf<PLACE>::type;
    const fr_text_run *runs = in.runs;
    const uint32_t n_runs = in.n_runs, n_places = in.n_places;
    const bool rgba = in.rgba;
    const bool srgb = (in.flags & FR_TEXT_SRGB) != 0, bgra = (in.flags & FR_TEXT_BGRA) != 0, load = (in.flags & FR_TEXT_LOAD) != 0;
    if (n_places && !places) return set_error(FR_E_INVALID, "places is NULL");
    if (n_runs && !runs) return set_error(FR_E_INVALID, "runs is NULL");
    if (rgba && n_places && !in.place_rgba) return set_error(FR_E_INVALID, "place_rgba is NULL");
    if (rgba && !load && n_runs && !in.run_clear_rgba) return set_error(FR_E_INVALID, "run_clear_rgba is NULL");
    if (in.n_glyphs && !in.boxes) return set_error(FR_E_INVALID, "text runs need the glyph boxes: fr_glyphset_set_boxes");
    // the runs and, run by run, their placements: each checked once; only the affine form keeps something for the build below
    std::vector<Inverse> inv(std::is_same<PLACE, fr_glyph_place_affine>::value ? n_places : 0);
    uint64_t pixels = 0, need_cols = 0, need_rows = 0, n_tiles = 0, n_refs = 0;
    for (uint32_t r = 0; r < n_runs; ++r) {
        const fr_text_run &rn = runs[r];
        if ((uint64_t)rn.first + rn.count > n_places) return set_error(FR_E_INVALID, "run %u: places %u + %u of %u", r, rn.first, rn.count, n_places);
        if (!(rn.scale > 0.0f) || !std::isfinite(rn.scale)) return set_error(FR_E_INVALID, "run %u: scale must be finite and > 0", r);
        if (rn.scale < 9.5367431640625e-07f || rn.scale > 1048576.0f) return set_error(FR_E_UNSUPPORTED, "run %u: scale outside [2^-20, 2^20]", r);
        if (rn.w > 65535u || rn.h > 65535u) return set_error(FR_E_UNSUPPORTED, "run %u: larger than 65535", r);
        for (uint32_t k = rn.first; k < rn.first + rn.count; ++k) {
            const Pen pen = pen_of(places[k]);
            if (pen.glyph >= in.n_glyphs) return set_error(FR_E_INVALID, "place %u: glyph %u of %u", k, pen.glyph, in.n_glyphs);
            if ((pen.x64 >> 6) < -LIM || (pen.x64 >> 6) > LIM || (pen.y64 >> 6) < -LIM || (pen.y64 >> 6) > LIM)
                return set_error(FR_E_UNSUPPORTED, "place %u: pen beyond +-2^22 pixels", k);
            if (const int rc = resolve(places[k], k, inv)) return rc;
        }
        pixels += (uint64_t)rn.w * rn.h;
        if (rn.w && rn.h) {
            n_refs += rn.count;
            need_cols = std::max<uint64_t>(need_cols, (uint64_t)rn.out_x + rn.w);
            need_rows = std::max<uint64_t>(need_rows, (uint64_t)rn.out_y + rn.h);
            n_tiles += (uint64_t)((rn.w + TEXT_TILE_W - 1) / TEXT_TILE_W) * ((rn.h + TEXT_TILE_H - 1) / TEXT_TILE_H);
        }
    }
    if (n_tiles > 0x7fffffffull) return set_error(FR_E_UNSUPPORTED, "text plan needs more than 2^31 workgroups; split it");
    // runs own their rectangles: no two may overlap (sweep down the rows)
    {
        std::vector<uint32_t> ord;
        for (uint32_t r = 0; r < n_runs; ++r)
            if (runs[r].w && runs[r].h) ord.push_back(r);
        std::sort(ord.begin(), ord.end(), [&](uint32_t a, uint32_t b) { return runs[a].out_y < runs[b].out_y; });
        for (size_t i = 0; i < ord.size(); ++i) {
            const fr_text_run &A = runs[ord[i]];
            for (size_t j = i + 1; j < ord.size() && runs[ord[j]].out_y < (uint64_t)A.out_y + A.h; ++j) {
                const fr_text_run &B = runs[ord[j]];
                if (B.out_x < (uint64_t)A.out_x + A.w && A.out_x < (uint64_t)B.out_x + B.w)
                    return set_error(FR_E_INVALID, "runs %u and %u overlap", ord[i], ord[j]);
            }
        }
    }
    // instances: each placement's cell (one column wider when fx != 0, one row taller when fy != 0) clipped to its run;
    // tiles: every 64 x 16 tile of every run, with the instances whose clipped cell meets it (counting sort by tile)
    out.runs.resize(n_runs);
    std::vector<TextTile> &tiles = out.tiles;
    tiles.resize((size_t)n_tiles);
    std::vector<INST> &insts = out.insts;
    std::vector<std::pair<uint32_t, uint32_t>> hits;            // (tile, instance)
    insts.reserve((size_t)std::min<uint64_t>(n_refs, n_places));   // (runs that share placements make the vectors grow past this)
    hits.reserve(insts.capacity());
    std::vector<uint8_t> used(in.n_glyphs, 0);
    uint32_t tbase = 0;
    for (uint32_t r = 0; r < n_runs; ++r) {
        const fr_text_run &rn = runs[r];
        const bool clear = rgba && !load;                                                  // (FR_TEXT_LOAD: no clear colour)
        out.runs[r] = TextRun{rn.w, rn.h, rn.out_x, rn.out_y, rn.scale, clear ? rgba_word(in.run_clear_rgba + 4 * (size_t)r, bgra) : 0u, {0, 0}};
        if (srgb) linear_words(out.runs[r].clear, out.runs[r].pad);
        if (!rn.w || !rn.h) continue;
        const uint32_t tx = (rn.w + TEXT_TILE_W - 1) / TEXT_TILE_W, ty = (rn.h + TEXT_TILE_H - 1) / TEXT_TILE_H;
        for (uint32_t y = 0; y < ty; ++y)
            for (uint32_t x = 0; x < tx; ++x)
                tiles[tbase + y * tx + x] = TextTile{r, x * TEXT_TILE_W, y * TEXT_TILE_H, 0, 0, {0, 0, 0}};
        for (uint32_t k = rn.first; k < rn.first + rn.count; ++k) {
            const Pen pen = pen_of(places[k]);
            const uint32_t g = pen.glyph;
            if (in.glyph_seg_start[g + 1] == in.glyph_seg_start[g]) continue;              // no segment: no winding anywhere
            const Cell c = cell_of(places[k], in.boxes + 4 * (size_t)g, rn.scale);
            const int64_t ix = pen.x64 >> 6, iy = pen.y64 >> 6;
            const uint32_t fx64 = (uint32_t)pen.x64 & 63u, fy64 = (uint32_t)pen.y64 & 63u;
            const int64_t cw = c.mxx - c.mnx + 1 + (fx64 ? 1 : 0), ch = c.mxy - c.mny + 1 + (fy64 ? 1 : 0);
            if (c.mnx < -LIM || c.mxx > LIM || c.mny < -LIM || c.mxy > LIM || cw > 65535 || ch > 65535)
                return set_error(FR_E_UNSUPPORTED, "place %u: cell beyond +-2^22 pixels or larger than 65535", k);
            const int64_t c0 = ix + c.mnx, r0 = iy - c.mxy;
            const int64_t x0 = std::max<int64_t>(c0, 0), x1 = std::min<int64_t>(c0 + cw, rn.w);
            const int64_t y0 = std::max<int64_t>(r0, 0), y1 = std::min<int64_t>(r0 + ch, rn.h);
            if (x0 >= x1 || y0 >= y1) continue;                                            // clipped away
            const uint32_t id = (uint32_t)insts.size();
            const uint32_t word = rgba ? rgba_word(in.place_rgba + 4 * (size_t)k, bgra) : 0u;
            insts.push_back(INST{(int32_t)ix, (int32_t)iy, (int32_t)x0, (int32_t)x1, (int32_t)y0, (int32_t)y1, g,
                                 2u * in.glyph_seg_start[g], fx64, word, {0, 0}});         // (the tail: zero until finish)
            if (srgb) linear_words(word, insts.back().pad);
            finish(insts.back(), places[k], inv, k, fy64, rn.scale);
            used[g] = 1;
            for (int64_t y = y0 / TEXT_TILE_H; y <= (y1 - 1) / TEXT_TILE_H; ++y)
                for (int64_t x = x0 / TEXT_TILE_W; x <= (x1 - 1) / TEXT_TILE_W; ++x)
                    hits.emplace_back(tbase + (uint32_t)(y * tx + x), id);
        }
        tbase += tx * ty;
    }
    if (hits.size() > 0xffffffffull) return set_error(FR_E_UNSUPPORTED, "text plan: too many tile / instance pairs; split it");
    out.list.resize(hits.size());
    for (const auto &h : hits) ++tiles[h.first].lend;
    uint32_t at = 0;
    for (auto &t : tiles) { t.lbeg = at; at += t.lend; t.lend = t.lbeg; }
    for (const auto &h : hits) out.list[tiles[h.first].lend++] = h.second;
    if (load)                          // FR_TEXT_LOAD: a tile no instance meets leaves its pixels as they are: not launched
        tiles.erase(std::remove_if(tiles.begin(), tiles.end(), [](const TextTile &t) { return t.lbeg == t.lend; }), tiles.end());
    for (uint32_t g = 0; g < in.n_glyphs; ++g)
        if (used[g]) out.glyphs.push_back(g);
    out.pixels = pixels; out.need_cols = need_cols; out.need_rows = need_rows;
    for (uint32_t k = 0; rgba && k < n_places; ++k)
        if (in.place_rgba[4 * (size_t)k + 3] != 255) { out.blend = (in.flags & FR_TEXT_OVER) ? 2 : 1; break; }
    return FR_OK;
}

template int text_plan_tables(const TextPlanIn &, const fr_glyph_place *, TextPlanTables<fr_glyph_place> &);
template int text_plan_tables(const TextPlanIn &, const fr_glyph_place_ex *, TextPlanTables<fr_glyph_place_ex> &);
template int text_plan_tables(const TextPlanIn &, const fr_glyph_place_affine *, TextPlanTables<fr_glyph_place_affine> &);

// ---- FR_TEXT_CACHE, FR_TEXT_CACHE_AFFINE (fr_text_plan.hpp) -----------------------------------------------------------
namespace {

uint32_t bits_of(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }

// what the key holds besides the glyph and the pen fractions, as bit patterns: the effective scale and the slant (the plain
// form is the _ex form at the run's scale, upright), or the four entries of the caller's matrix (equal m gives equal q)
using Shape = std::array<uint32_t, 4>;
Shape shape_of(const fr_glyph_place &, float run_scale) { return Shape{bits_of(run_scale), bits_of(0.0f), 0u, 0u}; }
Shape shape_of(const fr_glyph_place_ex &p, float run_scale) { return Shape{bits_of(scale_of(p, run_scale)), bits_of(p.slant), 0u, 0u}; }
Shape shape_of(const fr_glyph_place_affine &p, float) { return Shape{bits_of(p.m[0]), bits_of(p.m[1]), bits_of(p.m[2]), bits_of(p.m[3])}; }

// the cells of a form, and a key's cell record: the first instance `ti` of the key as an instance whose image is the whole
// cell (fr_text_tables.hpp), so that the tail of the record (scale and slant, or the inverse matrix) is the one finish wrote
std::vector<TextMaskCell> &cells_of(TextCacheTables &c, const TextInst *) { return c.cells; }
std::vector<TextMaskCell> &cells_of(TextCacheTables &c, const TextInstEx *) { return c.cells; }
std::vector<TextMaskCellAffine> &cells_of(TextCacheTables &c, const TextInstAffine *) { return c.acells; }
template <class INST>
TextInstEx whole_cell(const INST &ti, const Cell &c, int64_t cw, int64_t ch, uint32_t fy64, const Shape &sh)
{
    float scale, slant;
    std::memcpy(&scale, &sh[0], 4); std::memcpy(&slant, &sh[1], 4);
    return TextInstEx{(int32_t)-c.mnx, (int32_t)c.mxy, 0, (int32_t)cw, 0, (int32_t)ch, ti.glyph, ti.rec, ti.fx64, 0u, {0, 0}, fy64, scale, slant, 0u};
}
TextInstAffine whole_cell(const TextInstAffine &ti, const Cell &c, int64_t cw, int64_t ch, uint32_t fy64, const Shape &)
{
    return TextInstAffine{(int32_t)-c.mnx, (int32_t)c.mxy, 0, (int32_t)cw, 0, (int32_t)ch, ti.glyph, ti.rec, ti.fx64, 0u, {0, 0}, fy64,
                          ti.q00, ti.q01, ti.q10, ti.q11, {0, 0, 0}};
}

}  // namespace

// Walks the runs and placements exactly as text_plan_tables does, so that its k-th surviving placement is t.insts[k].
template <class PLACE>
int text_cache_tables(const TextPlanIn &in, const PLACE *places, const TextPlanTables<PLACE> &t, TextCacheTables &out)
{
    using Key = std::array<uint32_t, 7>;                   // glyph, fx64, fy64, the form's Shape
    using INST = typename TextInstOf<PLACE>::type;
    auto &cells = cells_of(out, (const INST *)nullptr);
    constexpr bool affine = std::is_same<PLACE, fr_glyph_place_affine>::value;
    std::map<Key, uint32_t> cell_of_key;
    out.insts.reserve(t.insts.size());
    uint64_t elems = 0;
    for (uint32_t r = 0; r < in.n_runs; ++r) {
        const fr_text_run &rn = in.runs[r];
        if (!rn.w || !rn.h) continue;
        for (uint32_t k = rn.first; k < rn.first + rn.count; ++k) {
            const Pen pen = pen_of(places[k]);
            const uint32_t g = pen.glyph;
            if (in.glyph_seg_start[g + 1] == in.glyph_seg_start[g]) continue;
            const Cell c = cell_of(places[k], in.boxes + 4 * (size_t)g, rn.scale);
            const int64_t ix = pen.x64 >> 6, iy = pen.y64 >> 6;
            const uint32_t fx64 = (uint32_t)pen.x64 & 63u, fy64 = (uint32_t)pen.y64 & 63u;
            const int64_t cw = c.mxx - c.mnx + 1 + (fx64 ? 1 : 0), ch = c.mxy - c.mny + 1 + (fy64 ? 1 : 0);
            const int64_t c0 = ix + c.mnx, r0 = iy - c.mxy;
            if (std::max<int64_t>(c0, 0) >= std::min<int64_t>(c0 + cw, rn.w) || std::max<int64_t>(r0, 0) >= std::min<int64_t>(r0 + ch, rn.h))
                continue;                                                                  // clipped away
            const size_t id = out.insts.size();
            if (id >= t.insts.size()) return set_error(FR_E_INVALID, "text cache: the tables are not those of these placements");
            const auto &ti = t.insts[id];
            const Shape sh = shape_of(places[k], rn.scale);
            const Key key{g, fx64, fy64, sh[0], sh[1], sh[2], sh[3]};
            auto it = cell_of_key.find(key);
            if (it == cell_of_key.end()) {
                if (elems + (uint64_t)(cw * ch) > TEXT_CACHE_MAX_ELEMS)
                    return set_error(FR_E_UNSUPPORTED, "%s: the mask cells hold more than 2^31 elements; split the plan or drop the flag",
                                     affine ? "FR_TEXT_CACHE_AFFINE" : "FR_TEXT_CACHE");
                typename std::remove_reference<decltype(cells)>::type::value_type mc{};
                mc.in = whole_cell(ti, c, cw, ch, fy64, sh);
                mc.base = (uint32_t)elems;
                elems += (uint64_t)(cw * ch);
                it = cell_of_key.emplace(key, (uint32_t)cells.size()).first;
                cells.push_back(mc);
            }
            const auto &mc = cells[it->second];
            out.insts.push_back(TextCachedInst{ti.x0, ti.x1, ti.y0, ti.y1, ti.rgba, {ti.pad[0], ti.pad[1]}, mc.base, (uint32_t)cw, (int32_t)c0, (int32_t)r0, 0u});
        }
    }
    if (out.insts.size() != t.insts.size()) return set_error(FR_E_INVALID, "text cache: the tables are not those of these placements");
    out.elems = elems;
    uint64_t n_tiles = 0;
    for (const auto &mc : cells)
        n_tiles += (uint64_t)((mc.in.x1 + TEXT_TILE_W - 1) / TEXT_TILE_W) * (uint64_t)((mc.in.y1 + TEXT_TILE_H - 1) / TEXT_TILE_H);
    if (n_tiles > 0x7fffffffull)
        return set_error(FR_E_UNSUPPORTED, "%s: the mask cells need more than 2^31 workgroups; split the plan", affine ? "FR_TEXT_CACHE_AFFINE" : "FR_TEXT_CACHE");
    out.tiles.reserve((size_t)n_tiles);
    for (uint32_t ci = 0; ci < cells.size(); ++ci)
        for (int32_t y = 0; y < cells[ci].in.y1; y += TEXT_TILE_H)
            for (int32_t x = 0; x < cells[ci].in.x1; x += TEXT_TILE_W)
                out.tiles.push_back(TextMaskTile{ci, (uint32_t)x, (uint32_t)y, 0u});
    return FR_OK;
}

template int text_cache_tables(const TextPlanIn &, const fr_glyph_place *, const TextPlanTables<fr_glyph_place> &, TextCacheTables &);
template int text_cache_tables(const TextPlanIn &, const fr_glyph_place_ex *, const TextPlanTables<fr_glyph_place_ex> &, TextCacheTables &);
template int text_cache_tables(const TextPlanIn &, const fr_glyph_place_affine *, const TextPlanTables<fr_glyph_place_affine> &, TextCacheTables &);

// ---- the launches of one render (fr_text_plan.hpp) --------------------------------------------------------------------
template <class PLACE>
TextPlan text_plan_of(const TextPlanIn &in, const fr_raster_params &params, const TextPlanTables<PLACE> &t, const TextCacheTables *cache)
{
    TextPlan p;
    p.form = text_form_of((const PLACE *)nullptr);
    p.rgba = in.rgba;
    p.srgb = in.rgba && (in.flags & FR_TEXT_SRGB) != 0;
    p.load = in.rgba && (in.flags & FR_TEXT_LOAD) != 0;
    p.blend = t.blend;
    p.fill = (in.flags & FR_FILL_CONSISTENT) ? 1 : 0;
    p.samples = params.samples_per_axis;
    p.n_tiles = (uint32_t)t.tiles.size(); p.n_insts = (uint32_t)t.insts.size(); p.n_glyphs = (uint32_t)t.glyphs.size();
    if (cache) {
        p.cached = true;
        p.n_mcells = (uint32_t)cache->n_cells(); p.n_mtiles = (uint32_t)cache->tiles.size();
    }
    return p;
}

template TextPlan text_plan_of(const TextPlanIn &, const fr_raster_params &, const TextPlanTables<fr_glyph_place> &, const TextCacheTables *);
template TextPlan text_plan_of(const TextPlanIn &, const fr_raster_params &, const TextPlanTables<fr_glyph_place_ex> &, const TextCacheTables *);
template TextPlan text_plan_of(const TextPlanIn &, const fr_raster_params &, const TextPlanTables<fr_glyph_place_affine> &, const TextCacheTables *);

// What a render launches and what fr_plan_describe prints are this one list.  The prepare and mask entries depend on their
// own counts and the last entry on the tiles, yet a plan without tiles launches nothing at all: it has no surviving
// instance (an instance meets at least one tile of its run, under FR_TEXT_LOAD too), hence no glyph to prepare and no mask
// cell.  A plan with tiles and no instance (not FR_TEXT_LOAD) still launches its text kernel, which writes the clear value.
void text_launches(const TextPlan &p, TextLaunchList &out)
{
    out.n = 0;
    if (p.n_glyphs) out.l[out.n++] = TextLaunch{TL_PREPARE, p.form, 0, p.samples, p.fill, 0, p.n_glyphs, p.n_glyphs};
    if (p.cached) out.l[out.n++] = TextLaunch{TL_MASK, p.form, 0, p.samples, p.fill, 0, p.n_mtiles, p.n_mcells};
    if (!p.n_tiles) return;
    const int colour = p.rgba ? 1 + (p.srgb ? 1 : 0) + (p.load ? 2 : 0) : 0;
    out.l[out.n++] = TextLaunch{p.cached ? TL_CACHED : TL_TEXT, p.form, colour, p.samples, p.cached ? 0 : p.fill, p.rgba ? p.blend : 0,
                                p.n_tiles, p.n_insts};
}

void text_launch_name(const TextLaunch &e, char *name, size_t cap)
{
    static const char *const form[3] = {"", "place_", "affine_"};
    static const char *const colour[5] = {"", "rgba_", "srgb_", "rgba_load_", "srgb_load_"};
    if (cap) name[0] = 0;
    if (e.fill != 0 && e.fill != 1) return;
    if (e.family == TL_PREPARE) { snprintf(name, cap, e.fill ? "fr::prepare_fill_kernel" : "fr::prepare_kernel"); return; }
    if (e.n != 1 && e.n != 2 && e.n != 4) return;
    if (e.family == TL_MASK) {
        snprintf(name, cap, e.form == TEXT_AFFINE ? "fr::glyph_mask_affine_kernel<%d, %d>" : "fr::glyph_mask_kernel<%d, %d>", e.n, e.fill);
        return;
    }
    if (e.colour < 0 || e.colour > 4 || e.blend < 0 || e.blend > 2 || (e.colour == 0 && e.blend != 0)) return;
    if (e.family == TL_CACHED) {
        if (e.colour == 0) snprintf(name, cap, "fr::text_cached_kernel<%d>", e.n);
        else snprintf(name, cap, "fr::text_cached_%skernel<%d, %d>", colour[e.colour], e.n, e.blend);
    } else if (e.form <= TEXT_AFFINE) {
        if (e.colour == 0) snprintf(name, cap, "fr::text_%skernel<%d, %d>", form[e.form], e.n, e.fill);
        else snprintf(name, cap, "fr::text_%s%skernel<%d, %d, %d>", form[e.form], colour[e.colour], e.n, e.fill, e.blend);
    }
}

}  // namespace fr

// text_cache_affine_selftest.cpp — the FR_TEXT_CACHE_AFFINE tables of matrix-form text plans (csrc/fr_text_plan.cpp:
// text_cache_tables for fr_glyph_place_affine) on the CPU: links fr_text_plan.o and nothing else of the library.  For a fixed
// list of small cases it prints the tables themselves, one line per case,
//   <case> insts .. cells .. tiles .. elems .. | C <cell>;.. | I <composite record>;.. | T <mask tile>;..
//     <cell>: glyph,fx64,fy64,ix,iy,cw,ch,rec,base,q00,q01,q10,q11 (the floats as bit patterns, in hex)
//     <composite record>: x0,x1,y0,y1,base,pitch,c0,r0        <mask tile>: cell,x0,y0
//   or   <case> error <code>: <message>
// and, as launches/<form>, the launch list of one cached plan per placement form.  tests/test_text_cache_affine_tables.py
// restates the key, the cell and the clipping in Python and compares (tests/golden/text_cache_affine_tables.json holds the
// cases and the lines).  By brute force it checks what glyph_mask_affine_kernel and the composites rely on:
//   - the cells' keys (glyph, both pen fractions, the bits of m) are unique, and every surviving instance reads the cell
//     of exactly its own key, whose record carries that instance's inverse matrix bit for bit;
//   - the cells' extents are back to back in the store and their sum is the reported total;
//   - every composite read of every pixel of every clipped cell lies inside the instance's cell extent (in the kernel's
//     own 32-bit arithmetic), at the pixel's offset from the unclipped cell's origin;
//   - the mask tiles cover every element of every cell exactly once by the stores the kernel makes, and every wave row
//     that reaches the record loop has its first lane inside the cell;
//   - beyond 2^31 elements the builder answers FR_E_UNSUPPORTED and has listed no tile.
// Exit status 1 if a property fails.
#include "../csrc/fr_text_plan.hpp"
#include "selftest.hpp"

#include <algorithm>
#include <array>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

using namespace selftest;

namespace {

// the glyph set of every case: boxes and segment counts only (glyph 2 has no segment; glyphs 3, 4 and 5 make cells of
// 1 x 1, 64 x 16 and 65 x 17 pixels under the identity; glyph 6 a cell of 40 001 x 40 001 at 1.25)
const int16_t BOXES[7][4] = {{2, -3, 20, 25}, {0, 0, 12, 16}, {1, 1, 9, 9}, {0, 0, 0, 0}, {0, 0, 63, 15}, {0, 0, 64, 16}, {0, 0, 32000, 32000}};
const uint32_t SEG_START[8] = {0, 4, 6, 6, 7, 10, 12, 13};
constexpr uint32_t N_GLYPHS = 7;

using Place = fr_glyph_place_affine;
struct Case {
    const char *name;
    std::vector<fr_text_run> runs;
    std::vector<Place> places;
};

fr_text_run run(uint32_t first, uint32_t count, uint32_t w, uint32_t h, uint32_t x, uint32_t y) { return fr_text_run{first, count, w, h, x, y, 1.0f}; }
struct M { float v[4]; };
Place at(uint32_t g, int32_t x64, int32_t y64, M m) { return Place{g, x64, y64, {m.v[0], m.v[1], m.v[2], m.v[3]}}; }

uint32_t bits_of(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
using Key = std::array<uint32_t, 7>;

void properties(const std::string &id, const std::vector<Place> &places, const std::vector<uint32_t> &survivor,
                const fr::TextPlanTables<Place> &t, const fr::TextCacheTables &c)
{
    const size_t ni = t.insts.size(), nc = c.acells.size();
    require(c.cells.empty(), id, "cells of the other forms' record");
    require(c.insts.size() == ni && survivor.size() == ni, id, "one composite record per instance");
    if (c.insts.size() != ni || survivor.size() != ni) return;
    uint64_t at = 0;
    for (const fr::TextMaskCellAffine &mc : c.acells) {
        const fr::TextInstAffine &in = mc.in;
        require(in.x0 == 0 && in.y0 == 0 && in.x1 > 0 && in.y1 > 0 && in.x1 <= 65535 && in.y1 <= 65535, id, "cell extent");
        require(mc.base == at, id, "cell extents are not disjoint and back to back");
        at += (uint64_t)in.x1 * (uint64_t)in.y1;
        require(in.glyph < N_GLYPHS && in.rec == 2u * SEG_START[in.glyph], id, "cell's first record");
        require(in.rgba == 0 && in.pad[0] == 0 && in.pad[1] == 0, id, "a cell has no colour");
    }
    require(at == c.elems && c.elems <= fr::TEXT_CACHE_MAX_ELEMS, id, "the extents' sum is not the reported total");
    // every instance against its placement: the cell it reads is the one whose first user had the same key
    std::vector<Key> keys(nc);
    std::vector<uint8_t> cell_used(nc, 0);
    for (size_t i = 0; i < ni; ++i) {
        const fr::TextInstAffine &in = t.insts[i];
        const fr::TextCachedInst &ci = c.insts[i];
        const Place &p = places[survivor[i]];
        const Key key{p.glyph, (uint32_t)p.pen_x64 & 63u, (uint32_t)p.pen_y64 & 63u, bits_of(p.m[0]), bits_of(p.m[1]), bits_of(p.m[2]), bits_of(p.m[3])};
        size_t cell = nc;
        for (size_t k = 0; k < nc; ++k)
            if (c.acells[k].base == ci.base) cell = k;
        require(cell < nc, id, "instance reads no cell's base");
        if (cell >= nc) continue;
        if (!cell_used[cell]) { keys[cell] = key; cell_used[cell] = 1; }
        require(keys[cell] == key, id, "instance does not read the cell of its own key");
        const fr::TextMaskCellAffine &mc = c.acells[cell];
        require(mc.in.glyph == in.glyph && mc.in.fx64 == in.fx64 && mc.in.fy64 == in.fy64 && bits_of(mc.in.q00) == bits_of(in.q00) &&
                bits_of(mc.in.q01) == bits_of(in.q01) && bits_of(mc.in.q10) == bits_of(in.q10) && bits_of(mc.in.q11) == bits_of(in.q11),
                id, "the cell's sample map is not the instance's");
        require(ci.pitch == (uint32_t)mc.in.x1, id, "pitch");
        require(ci.x0 == in.x0 && ci.x1 == in.x1 && ci.y0 == in.y0 && ci.y1 == in.y1 && ci.rgba == in.rgba && ci.pad[0] == in.pad[0] && ci.pad[1] == in.pad[1],
                id, "composite record differs from the instance");
        // the unclipped cell's origin: column 0 at ix + min_x, row 0 at iy - max_y (the cell holds ix = -min_x, iy = max_y)
        require(ci.c0 == in.ix - mc.in.ix && ci.r0 == in.iy - mc.in.iy, id, "cell origin");
        const uint64_t lo = mc.base, hi = lo + (uint64_t)mc.in.x1 * (uint64_t)mc.in.y1;
        for (int32_t Y = ci.y0; Y < ci.y1; ++Y)
            for (int32_t X = ci.x0; X < ci.x1; ++X) {
                const uint32_t addr = ci.base + (uint32_t)(Y - ci.r0) * ci.pitch + (uint32_t)(X - ci.c0);     // as the kernel computes it
                const int64_t dc = (int64_t)X - ci.c0, dr = (int64_t)Y - ci.r0;
                const bool ok = dc >= 0 && dc < mc.in.x1 && dr >= 0 && dr < mc.in.y1 && addr >= lo && addr < hi &&
                                (uint64_t)addr == lo + (uint64_t)dr * (uint64_t)mc.in.x1 + (uint64_t)dc;
                if (!ok) { require(false, id, "a composite read lies outside the instance's cell"); Y = ci.y1 - 1; break; }
            }
    }
    for (size_t k = 0; k < nc; ++k) require(cell_used[k] != 0, id, "a cell no instance reads");
    {
        std::vector<Key> s = keys;
        std::sort(s.begin(), s.end());
        require(std::adjacent_find(s.begin(), s.end()) == s.end(), id, "two cells share a key");
    }
    // the mask tiles: every element of every cell once, by the stores glyph_mask_affine_kernel makes
    std::vector<std::vector<uint8_t>> seen(nc);
    for (size_t k = 0; k < nc; ++k) seen[k].assign((size_t)c.acells[k].in.x1 * (size_t)c.acells[k].in.y1, 0);
    for (const fr::TextMaskTile &tl : c.tiles) {
        require(tl.cell < nc, id, "tile names no cell");
        if (tl.cell >= nc) continue;
        const fr::TextInstAffine &in = c.acells[tl.cell].in;
        require(tl.x0 % fr::TEXT_TILE_W == 0 && tl.y0 % fr::TEXT_TILE_H == 0 && (int64_t)tl.x0 < in.x1 && (int64_t)tl.y0 < in.y1, id, "tile origin");
        for (int yy = 0; yy < fr::TEXT_TILE_H; ++yy)
            for (int lane = 0; lane < fr::TEXT_TILE_W; ++lane) {
                const int X = (int)tl.x0 + lane, Y = (int)tl.y0 + yy;
                if (Y >= in.y1 || X >= in.x1) continue;                    // (the row's break, and `inside`)
                const uint32_t e = (uint32_t)Y * (uint32_t)in.x1 + (uint32_t)X;
                require(e < seen[tl.cell].size(), id, "a mask store lies outside its cell");
                if (e < seen[tl.cell].size()) ++seen[tl.cell][e];
            }
    }
    for (size_t k = 0; k < nc; ++k)
        require(std::all_of(seen[k].begin(), seen[k].end(), [](uint8_t v) { return v == 1; }), id, "the mask tiles do not cover a cell exactly once");
}

void run_case(const Case &c)
{
    const std::string id = c.name;
    fr::TextPlanIn in{};
    in.runs = c.runs.data();
    in.n_runs = (uint32_t)c.runs.size();
    in.n_places = (uint32_t)c.places.size();
    in.boxes = &BOXES[0][0];
    in.glyph_seg_start = SEG_START;
    in.n_glyphs = N_GLYPHS;
    fr::TextPlanTables<Place> t;
    clear_error();
    int rc = fr::text_plan_tables(in, c.places.data(), t);
    fr::TextCacheTables ct;
    if (rc == FR_OK) {
        rc = fr::text_cache_tables(in, c.places.data(), t, ct);
        if (rc != FR_OK) require(ct.tiles.empty(), id, "tiles listed although the builder failed");
    }
    if (rc != FR_OK) {
        printf("%s error %d: %s\n", id.c_str(), rc, last_error());
        return;
    }
    // which placement each instance is: the survivors in run and placement order, told by the instance's own fields
    std::vector<uint32_t> survivor;
    {
        size_t i = 0;
        for (const fr_text_run &rn : c.runs)
            for (uint32_t k = rn.first; k < rn.first + rn.count && rn.w && rn.h; ++k) {
                const Place &p = c.places[k];
                if (i < t.insts.size() && t.insts[i].glyph == p.glyph && t.insts[i].ix == (p.pen_x64 >> 6) && t.insts[i].iy == (p.pen_y64 >> 6) &&
                    t.insts[i].fx64 == ((uint32_t)p.pen_x64 & 63u) && t.insts[i].fy64 == ((uint32_t)p.pen_y64 & 63u)) {
                    survivor.push_back(k);
                    ++i;
                }
            }
    }
    properties(id, c.places, survivor, t, ct);
    std::string s = fmt("%s insts %zu cells %zu tiles %zu elems %llu | C", id.c_str(), ct.insts.size(), ct.acells.size(), ct.tiles.size(),
                        (unsigned long long)ct.elems);
    for (const fr::TextMaskCellAffine &mc : ct.acells) {
        const fr::TextInstAffine &a = mc.in;
        s += fmt(" %u,%u,%u,%d,%d,%d,%d,%u,%u,%08x,%08x,%08x,%08x;", a.glyph, a.fx64, a.fy64, a.ix, a.iy, a.x1, a.y1, a.rec, mc.base, bits_of(a.q00),
                 bits_of(a.q01), bits_of(a.q10), bits_of(a.q11));
    }
    s += " | I";
    for (const fr::TextCachedInst &ci : ct.insts) s += fmt(" %d,%d,%d,%d,%u,%u,%d,%d;", ci.x0, ci.x1, ci.y0, ci.y1, ci.base, ci.pitch, ci.c0, ci.r0);
    s += " | T";
    for (const fr::TextMaskTile &tl : ct.tiles) s += fmt(" %u,%u,%u;", tl.cell, tl.x0, tl.y0);
    puts(s.c_str());
}

// the launch list of a cached coverage plan (n = 4, FILL 0) of the form PLACE over one placement of glyph 1
template <class PLACE>
void launches(const char *form, const PLACE &place)
{
    const fr_text_run rn = run(0, 1, 40, 30, 0, 0);
    fr::TextPlanIn in{};
    in.runs = &rn; in.n_runs = 1; in.n_places = 1;
    in.boxes = &BOXES[0][0]; in.glyph_seg_start = SEG_START; in.n_glyphs = N_GLYPHS;
    fr::TextPlanTables<PLACE> t;
    fr::TextCacheTables ct;
    clear_error();
    const std::string id = std::string("launches/") + form;
    require(fr::text_plan_tables(in, &place, t) == FR_OK && fr::text_cache_tables(in, &place, t, ct) == FR_OK, id, "the builders failed");
    const fr_raster_params params{FR_COVERAGE_U8, 4, FR_SAMPLE_CENTER};
    fr::TextLaunchList L;
    fr::text_launches(fr::text_plan_of(in, params, t, ct.n_cells() ? &ct : nullptr), L);
    static const char *const family[4] = {"prepare", "mask", "text", "cached"};
    std::string s = id;
    for (uint32_t i = 0; i < L.n; ++i) {
        char name[96];
        fr::text_launch_name(L.l[i], name, sizeof name);
        s += fmt("%s %s %s x%u", i ? ";" : "", family[L.l[i].family], name, L.l[i].count);
    }
    puts(s.c_str());
}

}  // namespace

int main()
{
    const M H{{0.5f, 0.0f, 0.0f, 0.5f}}, SHEAR{{0.5f, 0.125f, 0.0f, 0.5f}}, NEGZ{{0.5f, -0.0f, 0.0f, 0.5f}}, QUARTER{{0.0f, -0.5f, 0.5f, 0.0f}},
        MIRROR{{-0.5f, 0.0f, 0.0f, 0.5f}}, ONE{{1.0f, 0.0f, 0.0f, 1.0f}}, BIG{{1.25f, 0.0f, 0.0f, 1.25f}}, TURN{{0.3535534f, -0.3535534f, 0.3535534f, 0.3535534f}};
    std::vector<Case> cases;
    auto add = [&](const char *name, std::vector<fr_text_run> runs, std::vector<Place> places) { cases.push_back(Case{name, std::move(runs), std::move(places)}); };
    auto R = [&](uint32_t count) { return std::vector<fr_text_run>{run(0, count, 40, 30, 3, 5)}; };
    // one key at two whole pens: one cell, two composite records
    add("one_key_two_pens", R(2), {at(0, 5 * 64 + 17, 20 * 64 + 9, H), at(0, 12 * 64 + 17, 22 * 64 + 9, H)});
    add("two_matrices", R(3), {at(0, 5 * 64, 20 * 64, H), at(0, 15 * 64, 20 * 64, SHEAR), at(0, 22 * 64, 22 * 64, H)});
    add("signed_zero", R(2), {at(1, 5 * 64, 20 * 64, H), at(1, 20 * 64, 20 * 64, NEGZ)});
    add("fractions", R(5), {at(1, 5 * 64, 12 * 64, H), at(1, 15 * 64 + 8, 12 * 64, H), at(1, 25 * 64, 12 * 64 + 8, H), at(1, 5 * 64 + 8, 24 * 64 + 8, H),
                            at(1, 15 * 64 + 8, 24 * 64 + 8, H)});
    add("quarter_mirror_turn", R(4), {at(0, 20 * 64, 20 * 64, QUARTER), at(0, 30 * 64 + 5, 20 * 64, MIRROR), at(0, 20 * 64, 25 * 64 + 63, TURN), at(0, 35 * 64, 10 * 64, QUARTER)});
    // half outside the run at its right and bottom edges, and at its left and top: the cell is whole, x0 .. y1 are clipped
    add("half_outside", R(2), {at(0, 35 * 64 + 3, 33 * 64 + 3, H), at(0, -5 * 64 + 3, 2 * 64 + 3, H)});
    add("skipped_between", R(5), {at(0, 5 * 64, 20 * 64, H), at(0, 1000 * 64, 20 * 64, H), at(2, 6 * 64, 20 * 64, H), at(1, 10 * 64, -400 * 64, H), at(0, 20 * 64, 21 * 64, H)});
    add("no_segments", R(1), {at(2, 6 * 64, 20 * 64, H)});
    add("clipped_away", R(2), {at(0, 1000 * 64, 20 * 64, H), at(2, 6 * 64, 20 * 64, H)});
    add("no_runs", {}, {at(0, 5 * 64, 20 * 64, H)});
    // cell tiles: cw in {1, 64, 65} and ch in {1, 16, 17}, and 2 x 2
    add("tiles", {run(0, 6, 200, 60, 0, 0)}, {at(3, 2 * 64, 3 * 64, ONE), at(4, 5 * 64, 20 * 64, ONE), at(5, 70 * 64, 20 * 64, ONE), at(4, 5 * 64 + 1, 40 * 64, ONE),
                                              at(4, 70 * 64, 40 * 64 + 1, ONE), at(3, 150 * 64 + 32, 50 * 64 + 32, ONE)});
    // two runs: the second shares the first's key, and has one of its own
    add("two_runs", {run(0, 2, 40, 30, 0, 0), run(2, 2, 64, 16, 40, 0)}, {at(0, 5 * 64, 20 * 64, H), at(1, 20 * 64, 25 * 64, H), at(0, 9 * 64, 14 * 64, H), at(1, 30 * 64, 12 * 64, SHEAR)});
    // the store's limit: two keys whose cells hold 40001 x 40001 elements (and one column more) each; one alone is within it
    add("err_store_cap", {run(0, 2, 100, 100, 0, 0)}, {at(6, 0, 50 * 64, BIG), at(6, 1, 50 * 64, BIG)});
    add("one_huge_cell", {run(0, 2, 100, 100, 0, 0)}, {at(6, 0, 50 * 64, BIG), at(6, 64, 51 * 64, BIG)});
    for (const Case &c : cases) {
        if (std::string(c.name) == "one_huge_cell") {                      // (its tables are not printed: 1.6e9 elements in 1.6e6 tiles)
            fr::TextPlanIn in{};
            in.runs = c.runs.data(); in.n_runs = 1; in.n_places = 2;
            in.boxes = &BOXES[0][0]; in.glyph_seg_start = SEG_START; in.n_glyphs = N_GLYPHS;
            fr::TextPlanTables<Place> t;
            fr::TextCacheTables ct;
            const int rc = fr::text_plan_tables(in, c.places.data(), t) ? -100 : fr::text_cache_tables(in, c.places.data(), t, ct);
            printf("%s rc %d insts %zu cells %zu elems %llu\n", c.name, rc, ct.insts.size(), ct.acells.size(), (unsigned long long)ct.elems);
            continue;
        }
        run_case(c);
    }
    launches("affine", at(1, 5 * 64, 20 * 64, H));
    launches("ex", fr_glyph_place_ex{1, 5 * 64, 20 * 64, 0.5f, 0.0f});
    launches("plain", fr_glyph_place{1, 5 * 64, 20});
    return exit_status();
}

// text_cache_selftest.cpp — the FR_TEXT_CACHE tables of text plans (csrc/fr_text_plan.cpp: text_cache_tables) on the CPU:
// links fr_text_plan.o and nothing else of the library.  For a fixed list of small cases in both cacheable placement
// forms it prints one line per case and form,
//   <case>/<form> <FNV-1a 64 of the three tables and the element count> insts .. cells .. tiles .. elems ..
//   or   <case>/<form> error <code>: <message>
// which tests/test_text_cache_tables.py compares with tests/golden/text_cache_tables.json, and checks by brute force what
// the kernels of csrc/fr_text_cached.hip rely on:
//   - the cells' keys are unique, and every surviving instance reads the cell of exactly its own key;
//   - the cells' extents are disjoint in the store and their sum is the reported total;
//   - for every instance and every pixel of its clipped cell, the element the composite kernel would read (computed in
//     the kernel's own 32-bit arithmetic) lies inside that instance's cell extent, at the pixel's offset from the
//     unclipped cell's origin;
//   - the mask tiles cover every element of every cell exactly once, and every store of glyph_mask_kernel is in range;
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

// the glyph set of every case: boxes and segment counts only (glyph 3 has no segment; glyph 5's box makes cells of more
// than 2^30 elements at scale 1.25)
const int16_t BOXES[6][4] = {{2, -3, 20, 25}, {0, 0, 12, 16}, {-5, -8, 30, 40}, {1, 1, 9, 9}, {0, -10, 100, 90}, {0, 0, 32000, 32000}};
const uint32_t SEG_START[7] = {0, 4, 6, 13, 13, 18, 19};
enum { PLAIN = 1, EX = 2, BOTH = 3 };

struct Place { uint32_t glyph; int32_t pen_x64, pen_y64; float scale, slant; };
struct Case {
    const char *name;
    int forms;
    uint32_t flags;                    // FR_TEXT_LOAD makes an RGBA case
    std::vector<fr_text_run> runs;
    std::vector<Place> places;
};

fr_text_run run(uint32_t first, uint32_t count, uint32_t w, uint32_t h, uint32_t x, uint32_t y, float s) { return fr_text_run{first, count, w, h, x, y, s}; }
Place at(uint32_t g, int32_t x64, int32_t y64, float scale = 0.0f, float slant = 0.0f) { return Place{g, x64, y64, scale, slant}; }
fr_glyph_place convert(const Place &p, const fr_glyph_place *) { return fr_glyph_place{p.glyph, p.pen_x64, p.pen_y64 >> 6}; }
fr_glyph_place_ex convert(const Place &p, const fr_glyph_place_ex *) { return fr_glyph_place_ex{p.glyph, p.pen_x64, p.pen_y64, p.scale, p.slant}; }

struct Fnv {
    uint64_t h = 0xcbf29ce484222325ull;
    void bytes(const void *p, size_t n)
    {
        for (size_t i = 0; i < n; ++i) h = (h ^ static_cast<const unsigned char *>(p)[i]) * 0x100000001b3ull;
    }
    void u64(uint64_t v) { bytes(&v, 8); }
    template <class T> void vec(const std::vector<T> &v) { u64(v.size()); bytes(v.data(), v.size() * sizeof(T)); }
};

uint32_t bits_of(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
using Key = std::array<uint32_t, 5>;

// an instance's key from the plan's own tables: the run's scale for the upright form, the placement's fields for _ex
Key key_of(const fr::TextInst &in, const fr::TextRun &r) { return Key{in.glyph, in.fx64, 0u, bits_of(r.scale), bits_of(0.0f)}; }
Key key_of(const fr::TextInstEx &in, const fr::TextRun &) { return Key{in.glyph, in.fx64, in.fy64, bits_of(in.scale), bits_of(in.slant)}; }
int32_t iy_of(const fr::TextInst &in) { return in.pen_y; }
int32_t iy_of(const fr::TextInstEx &in) { return in.iy; }

template <class PLACE>
void properties(const std::string &id, const fr::TextPlanTables<PLACE> &t, const fr::TextCacheTables &c)
{
    const size_t ni = t.insts.size(), nc = c.cells.size();
    require(c.insts.size() == ni, id, "one composite record per instance");
    if (c.insts.size() != ni) return;
    // the cells: unique keys, extents back to back from 0 to elems
    std::vector<Key> keys;
    uint64_t at = 0;
    for (const fr::TextMaskCell &mc : c.cells) {
        const fr::TextInstEx &in = mc.in;
        keys.push_back(Key{in.glyph, in.fx64, in.fy64, bits_of(in.scale), bits_of(in.slant)});
        require(in.x0 == 0 && in.y0 == 0 && in.x1 > 0 && in.y1 > 0 && in.x1 <= 65535 && in.y1 <= 65535, id, "cell extent");
        require(mc.base == at, id, "cell extents are not disjoint and back to back");
        at += (uint64_t)in.x1 * (uint64_t)in.y1;
        require(in.rec == 2u * SEG_START[in.glyph], id, "cell's first record");
    }
    require(at == c.elems && c.elems <= fr::TEXT_CACHE_MAX_ELEMS, id, "the extents' sum is not the reported total");
    {
        std::vector<Key> s = keys;
        std::sort(s.begin(), s.end());
        require(std::adjacent_find(s.begin(), s.end()) == s.end(), id, "two cells share a key");
    }
    // each instance's run, from the tiles that list it
    std::vector<int64_t> inst_run(ni, -1);
    for (const auto &tl : t.tiles)
        for (uint32_t k = tl.lbeg; k < tl.lend; ++k) inst_run[t.list[k]] = tl.run;
    std::vector<uint8_t> cell_used(nc, 0);
    for (size_t i = 0; i < ni; ++i) {
        const auto &in = t.insts[i];
        const fr::TextCachedInst &ci = c.insts[i];
        require(inst_run[i] >= 0, id, "instance in no tile's list");
        if (inst_run[i] < 0) continue;
        const Key want = key_of(in, t.runs[(size_t)inst_run[i]]);
        const size_t cell = (size_t)(std::find(keys.begin(), keys.end(), want) - keys.begin());
        require(cell < nc, id, "no cell has the instance's key");
        if (cell >= nc) continue;
        cell_used[cell] = 1;
        const fr::TextMaskCell &mc = c.cells[cell];
        const uint64_t lo = mc.base, hi = lo + (uint64_t)mc.in.x1 * (uint64_t)mc.in.y1;
        require(ci.base == mc.base && ci.pitch == (uint32_t)mc.in.x1, id, "instance does not read the cell of its own key");
        require(ci.x0 == in.x0 && ci.x1 == in.x1 && ci.y0 == in.y0 && ci.y1 == in.y1 && ci.rgba == in.rgba && ci.pad[0] == in.pad[0] && ci.pad[1] == in.pad[1],
                id, "composite record differs from the instance");
        // the unclipped cell's origin: column 0 at ix + min_x, row 0 at iy - max_y (the cell holds ix = -min_x, iy = max_y)
        require(ci.c0 == in.ix - mc.in.ix && ci.r0 == iy_of(in) - mc.in.iy, id, "cell origin");
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
    // the mask tiles: every element of every cell once, by the stores glyph_mask_kernel makes
    std::vector<std::vector<uint8_t>> seen(nc);
    for (size_t k = 0; k < nc; ++k) seen[k].assign((size_t)c.cells[k].in.x1 * (size_t)c.cells[k].in.y1, 0);
    for (const fr::TextMaskTile &tl : c.tiles) {
        require(tl.cell < nc, id, "tile names no cell");
        if (tl.cell >= nc) continue;
        const fr::TextInstEx &in = c.cells[tl.cell].in;
        require(tl.x0 % fr::TEXT_TILE_W == 0 && tl.y0 % fr::TEXT_TILE_H == 0 && (int64_t)tl.x0 < in.x1 && (int64_t)tl.y0 < in.y1, id, "tile origin");
        for (int yy = 0; yy < fr::TEXT_TILE_H; ++yy)
            for (int lane = 0; lane < fr::TEXT_TILE_W; ++lane) {
                const int X = (int)tl.x0 + lane, Y = (int)tl.y0 + yy;
                if (Y >= in.y1 || X >= in.x1) continue;                    // (the kernel's two guards)
                const uint32_t e = (uint32_t)Y * (uint32_t)in.x1 + (uint32_t)X;
                require(e < seen[tl.cell].size(), id, "a mask store lies outside its cell");
                if (e < seen[tl.cell].size()) ++seen[tl.cell][e];
            }
    }
    for (size_t k = 0; k < nc; ++k)
        require(std::all_of(seen[k].begin(), seen[k].end(), [](uint8_t v) { return v == 1; }), id, "the mask tiles do not cover a cell exactly once");
}

template <class PLACE>
void run_form(const Case &c, const char *form)
{
    const std::string id = std::string(c.name) + "/" + form;
    std::vector<PLACE> places;
    for (const Place &p : c.places) places.push_back(convert(p, (const PLACE *)nullptr));
    const bool rgba = (c.flags & FR_TEXT_LOAD) != 0;
    std::vector<uint8_t> colours;
    for (size_t k = 0; k < 4 * places.size(); ++k) colours.push_back((uint8_t)(k % 4 == 3 ? 255 : 40 + 9 * k));
    fr::TextPlanIn in{};
    in.runs = c.runs.data();
    in.n_runs = (uint32_t)c.runs.size();
    in.n_places = (uint32_t)places.size();
    in.place_rgba = rgba ? colours.data() : nullptr;
    in.rgba = rgba;
    in.flags = c.flags;
    in.boxes = &BOXES[0][0];
    in.glyph_seg_start = SEG_START;
    in.n_glyphs = 6;
    fr::TextPlanTables<PLACE> t;
    clear_error();
    int rc = fr::text_plan_tables(in, places.data(), t);
    fr::TextCacheTables ct;
    if (rc == FR_OK) {
        rc = fr::text_cache_tables(in, places.data(), t, ct);
        if (rc != FR_OK) require(ct.tiles.empty(), id, "tiles listed although the builder failed");
    }
    if (rc != FR_OK) {
        printf("%s error %d: %s\n", id.c_str(), rc, last_error());
        return;
    }
    properties(id, t, ct);
    Fnv f;
    f.vec(ct.cells); f.vec(ct.tiles); f.vec(ct.insts); f.u64(ct.elems);
    printf("%s %016llx insts %zu cells %zu tiles %zu elems %llu\n", id.c_str(), (unsigned long long)f.h, ct.insts.size(), ct.cells.size(),
           ct.tiles.size(), (unsigned long long)ct.elems);
}

void run_case(const Case &c)
{
    if (c.forms & PLAIN) run_form<fr_glyph_place>(c, "plain");
    if (c.forms & EX) run_form<fr_glyph_place_ex>(c, "ex");
}

}  // namespace

int main()
{
    const float S = 0.5f;
    std::vector<Case> cases;
    auto add = [&](const char *name, int forms, std::vector<fr_text_run> runs, std::vector<Place> places, uint32_t flags = 0u) {
        cases.push_back(Case{name, forms, flags, std::move(runs), std::move(places)});
    };
    auto R = [&](uint32_t count, float s = 0.5f) { return std::vector<fr_text_run>{run(0, count, 40, 30, 3, 5, s)}; };
    // sharing: the same glyph at the same fraction three times (one cell), once at another fraction, and another glyph
    add("shared", BOTH, R(5), {at(0, 5 * 64 + 17, 20 * 64), at(0, 12 * 64 + 17, 22 * 64), at(1, 20 * 64, 25 * 64), at(0, 17, 9 * 64), at(0, 9 * 64 + 18, 20 * 64)});
    add("no_sharing", BOTH, R(3), {at(0, 5 * 64, 20 * 64), at(1, 20 * 64, 25 * 64), at(2, 10 * 64, 22 * 64)});
    // pairs that differ in exactly one key field, and two identical placements: 6 cells for 7 instances
    add("one_field_each", EX, R(7), {at(1, 10 * 64 + 8, 20 * 64 + 8, 0.5f, 0.25f), at(2, 10 * 64 + 8, 20 * 64 + 8, 0.5f, 0.25f),
                                     at(1, 10 * 64 + 9, 20 * 64 + 8, 0.5f, 0.25f), at(1, 10 * 64 + 8, 20 * 64 + 9, 0.5f, 0.25f),
                                     at(1, 10 * 64 + 8, 20 * 64 + 8, 0.75f, 0.25f), at(1, 10 * 64 + 8, 20 * 64 + 8, 0.5f, -0.25f),
                                     at(1, 20 * 64 + 8, 24 * 64 + 8, 0.5f, 0.25f)});
    add("glyph_or_fraction", PLAIN, R(4), {at(1, 10 * 64 + 8, 20 * 64), at(2, 10 * 64 + 8, 20 * 64), at(1, 10 * 64 + 9, 20 * 64), at(1, 25 * 64 + 8, 21 * 64)});
    // scale 0 is the run's scale: one key with an explicit 0.5; slant 0.0 and -0.0 are two keys
    add("effective_scale", EX, R(4), {at(1, 5 * 64, 20 * 64), at(1, 20 * 64, 20 * 64, 0.5f), at(1, 5 * 64, 28 * 64, 0.0f, -0.0f), at(1, 20 * 64, 28 * 64, 0.25f)});
    // two runs of one scale share cells; a third of another scale does not
    add("three_runs", BOTH, {run(0, 2, 40, 30, 0, 0, S), run(2, 2, 40, 30, 40, 0, S), run(4, 2, 40, 30, 80, 0, 0.75f)},
        {at(0, 5 * 64, 20 * 64), at(1, 20 * 64 + 3, 25 * 64), at(0, 9 * 64, 21 * 64), at(1, 3, 25 * 64), at(0, 5 * 64, 20 * 64), at(1, 20 * 64 + 3, 25 * 64)});
    add("two_runs_shared_places", BOTH, {run(0, 3, 40, 30, 0, 40, S), run(1, 2, 64, 16, 0, 0, S)}, {at(0, 5 * 64, 20 * 64), at(1, 20 * 64, 25 * 64), at(2, 10 * 64, 22 * 64)});
    // clipping at every edge, negative pens, and placements clipped away or without segments between shared ones
    add("clipped_each_side", BOTH, {run(0, 6, 30, 30, 0, 0, S)},
        {at(1, -3 * 64, 15 * 64), at(1, 27 * 64, 15 * 64), at(1, 10 * 64, 3 * 64), at(1, 10 * 64, 33 * 64), at(4, -10 * 64, 40 * 64), at(4, -10 * 64 - 64, 41 * 64)});
    add("pen_negative", BOTH, R(3), {at(4, -100, 20 * 64), at(2, 3 * 64, -70), at(0, -1, -1 + 12 * 64)});
    add("skipped_between", BOTH, R(5), {at(0, 1000 * 64, 20 * 64), at(1, 20 * 64, 25 * 64), at(3, 6 * 64, 20 * 64), at(2, 10 * 64, -400 * 64), at(1, 4 * 64, 20 * 64)});
    add("clipped_away", BOTH, R(2), {at(0, 1000 * 64, 20 * 64), at(3, 6 * 64, 20 * 64)});
    add("no_runs", BOTH, {}, {at(0, 5 * 64, 20 * 64)});
    // cells of several mask tiles: 100 x 90 font units at scale 1.5 (151 x 151 pixels, 152 with a fraction), twice
    add("large_cell", BOTH, {run(0, 3, 400, 200, 0, 0, 1.5f)}, {at(4, 10 * 64, 150 * 64), at(4, 200 * 64 + 32, 140 * 64), at(4, 100 * 64 + 32, 199 * 64)});
    add("slanted_large", EX, {run(0, 2, 300, 100, 0, 0, S)}, {at(4, 20 * 64 + 5, 60 * 64 + 7, 0.75f, 4.0f), at(4, 150 * 64 + 5, 70 * 64 + 7, 0.75f, 4.0f)});
    add("load_empty_tiles", BOTH, {run(0, 3, 200, 40, 7, 9, S)}, {at(0, 5 * 64, 20 * 64), at(1, 20 * 64, 25 * 64), at(0, 150 * 64, 20 * 64)}, FR_TEXT_LOAD);
    // the store's limit: two keys whose cells hold 40001 x 40001 elements each; one such cell alone is within it
    add("err_store_cap", BOTH, {run(0, 2, 100, 100, 0, 0, 1.25f)}, {at(5, 0, 50 * 64), at(5, 1, 50 * 64)});
    for (const Case &c : cases) run_case(c);
    return exit_status();
}

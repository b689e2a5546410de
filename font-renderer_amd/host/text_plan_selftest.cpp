// text_plan_selftest.cpp — the table builder of text plans (csrc/fr_text_plan.cpp) on the CPU: links fr_text_plan.o and
// nothing else of the library.  For a fixed list of small cases it prints one line per case and placement form,
//   <case>/<form> <FNV-1a 64 of every returned vector and scalar> <the vectors' lengths>   or   <case>/<form> error <code>: <message>
// which tests/test_text_plan_tables.py compares with tests/golden/text_plan_tables.json, and checks by brute force, with
// no tolerance, what the kernels rely on: every cell inside its run, every tile's list exactly the instances that meet
// it and in placement order, no empty tile under FR_TEXT_LOAD, the glyph list sorted and exact.  Exit status 1 if a
// property fails.  The one message without a case is "too many tile / instance pairs" (more than 2^32 of them).
// With the argument "over" it runs the FR_TEXT_OVER cases instead (tests/test_text_over_ref.py): each RGBA case with and
// without the flag, one line each ending in "blend <0|1|2>", the hash taken over everything but the blend value, and
// checks that the flag changes nothing but that value: 2 in place of 1, 0 where every colour is opaque.
// With the argument "launches" it prints the launch list of a handful of plans (tests/test_text_launches.py): per form
// "<case>/<form>/launches <n>" and per entry "<case>/<form>/launch<i> <family> <kernel name> grid <workgroups> count <what
// fr_plan_describe prints>", then text_launch_name over a box of keys: one "name/..." line per key that has a kernel.
// In every mode each plan's list is checked against what the render and the description rely on (launch_properties).
#include "../csrc/fr_text_plan.hpp"
#include "selftest.hpp"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <type_traits>
#include <vector>

using namespace selftest;

namespace {

// the glyph set of every case: boxes and segment counts only (glyph 3 has no segment, glyph 5 is never placed)
const int16_t BOXES[6][4] = {{2, -3, 20, 25}, {0, 0, 12, 16}, {-5, -8, 30, 40}, {1, 1, 9, 9}, {0, -10, 100, 90}, {0, 0, 4, 4}};
const uint32_t SEG_START[7] = {0, 4, 6, 13, 13, 18, 19};
enum { PLAIN = 1, EX = 2, AFFINE = 4, ALL = 7 };

struct Place {                         // a placement in the widest terms; each form takes what it has
    uint32_t glyph;
    int32_t pen_x64, pen_y64;
    float scale, slant;                // fr_glyph_place_ex; the affine form takes m, or {s, s * slant, 0, s} when m is all 0
    float m[4];
};
struct Case {
    const char *name;
    int forms;
    bool rgba;
    uint32_t flags;
    float scale;                       // of every run
    std::vector<fr_text_run> runs;
    std::vector<Place> places;
    std::vector<uint8_t> colours, clears;
    bool null_places = false, null_runs = false, no_boxes = false;
    int samples = 4;                   // per axis (launches)
};

fr_text_run run(uint32_t first, uint32_t count, uint32_t w, uint32_t h, uint32_t x, uint32_t y, float s) { return fr_text_run{first, count, w, h, x, y, s}; }
Place at(uint32_t g, int32_t x64, int32_t y64, float scale = 0.0f, float slant = 0.0f) { return Place{g, x64, y64, scale, slant, {0, 0, 0, 0}}; }
Place mat(uint32_t g, int32_t x64, int32_t y64, float xx, float xy, float yx, float yy) { return Place{g, x64, y64, 0.0f, 0.0f, {xx, xy, yx, yy}}; }

fr_glyph_place convert(const Place &p, float, const fr_glyph_place *) { return fr_glyph_place{p.glyph, p.pen_x64, p.pen_y64 >> 6}; }
fr_glyph_place_ex convert(const Place &p, float, const fr_glyph_place_ex *) { return fr_glyph_place_ex{p.glyph, p.pen_x64, p.pen_y64, p.scale, p.slant}; }
fr_glyph_place_affine convert(const Place &p, float run_scale, const fr_glyph_place_affine *)
{
    const float s = p.scale != 0.0f ? p.scale : run_scale;
    const bool own = p.m[0] != 0.0f || p.m[1] != 0.0f || p.m[2] != 0.0f || p.m[3] != 0.0f;
    if (own) return fr_glyph_place_affine{p.glyph, p.pen_x64, p.pen_y64, {p.m[0], p.m[1], p.m[2], p.m[3]}};
    return fr_glyph_place_affine{p.glyph, p.pen_x64, p.pen_y64, {s, s * p.slant, 0.0f, s}};
}

struct Fnv {
    uint64_t h = 0xcbf29ce484222325ull;
    void bytes(const void *p, size_t n)
    {
        for (size_t i = 0; i < n; ++i) h = (h ^ static_cast<const unsigned char *>(p)[i]) * 0x100000001b3ull;
    }
    void u64(uint64_t v) { bytes(&v, 8); }
    template <class T> void vec(const std::vector<T> &v) { u64(v.size()); bytes(v.data(), v.size() * sizeof(T)); }
};

template <class PLACE>
void properties(const std::string &id, const Case &c, const fr::TextPlanTables<PLACE> &t)
{
    const bool load = c.rgba && (c.flags & FR_TEXT_LOAD);
    const size_t ni = t.insts.size();
    // the tile lists partition `list`; an instance belongs to the run of the tiles that list it, and the instances lie in run order
    std::vector<int64_t> inst_run(ni, -1);
    uint32_t at = 0;
    for (const auto &tl : t.tiles) {
        require(tl.lbeg == at && tl.lend >= tl.lbeg && tl.lend <= t.list.size(), id, "tile lists do not partition the list");
        at = tl.lend;
        require(!load || tl.lend > tl.lbeg, id, "empty tile listed under FR_TEXT_LOAD");
        for (uint32_t k = tl.lbeg; k < tl.lend && k < t.list.size(); ++k) {
            const uint32_t i = t.list[k];
            require(i < ni, id, "list names no instance");
            if (i >= ni) continue;
            require(k == tl.lbeg || t.list[k - 1] < i, id, "a tile's list is not in placement order");
            require(inst_run[i] < 0 || inst_run[i] == (int64_t)tl.run, id, "instance listed by two runs");
            inst_run[i] = tl.run;
        }
    }
    require(at == t.list.size(), id, "list longer than the tiles' ranges");
    require(t.runs.size() == c.runs.size(), id, "run count");
    for (size_t i = 0; i < ni; ++i) {
        const auto &in = t.insts[i];
        require(inst_run[i] >= 0, id, "instance in no tile's list");
        if (inst_run[i] < 0) continue;
        require(i == 0 || inst_run[i - 1] <= inst_run[i], id, "instances not in run order");
        const fr::TextRun &r = t.runs[(size_t)inst_run[i]];
        require(0 <= in.x0 && in.x0 < in.x1 && in.x1 <= (int64_t)r.w && 0 <= in.y0 && in.y0 < in.y1 && in.y1 <= (int64_t)r.h, id,
                "instance cell not inside its run");
    }
    // every tile of every run, in order: listed (without LOAD always), and its list is exactly the run's instances that meet it
    size_t k = 0;
    for (size_t r = 0; r < t.runs.size(); ++r)
        for (uint32_t y0 = 0; y0 < t.runs[r].h && t.runs[r].w; y0 += fr::TEXT_TILE_H)
            for (uint32_t x0 = 0; x0 < t.runs[r].w; x0 += fr::TEXT_TILE_W) {
                std::vector<uint32_t> want;
                for (size_t i = 0; i < ni; ++i) {
                    const auto &in = t.insts[i];
                    if (inst_run[i] == (int64_t)r && in.x0 < (int64_t)x0 + fr::TEXT_TILE_W && in.x1 > (int64_t)x0 &&
                        in.y0 < (int64_t)y0 + fr::TEXT_TILE_H && in.y1 > (int64_t)y0)
                        want.push_back((uint32_t)i);
                }
                const bool here = k < t.tiles.size() && t.tiles[k].run == r && t.tiles[k].x0 == x0 && t.tiles[k].y0 == y0;
                if (!here) {
                    require(load && want.empty(), id, "a tile is missing");
                    continue;
                }
                const auto &tl = t.tiles[k++];
                const std::vector<uint32_t> got(t.list.begin() + tl.lbeg, t.list.begin() + std::min<size_t>(tl.lend, t.list.size()));
                require(got == want, id, "a tile's list is not the instances whose cell meets it");
            }
    require(k == t.tiles.size(), id, "tiles that belong to no run");
    std::vector<uint32_t> used;
    for (const auto &in : t.insts) used.push_back(in.glyph);
    std::sort(used.begin(), used.end());
    used.erase(std::unique(used.begin(), used.end()), used.end());
    require(used == t.glyphs, id, "glyph list not sorted and exact");
}

// what the render and fr_plan_describe rely on when they walk one list (text_launches, csrc/fr_text_plan.cpp): a plan without
// tiles has no instance, no glyph and no mask cell, so its list is empty; any other list ends in the text kernel or the
// composite over the plan's tiles; the entries come in stream order, each with a kernel name
void launch_properties(const std::string &id, const fr::TextPlan &p, const fr::TextLaunchList &L)
{
    if (!p.n_tiles) require(!p.n_insts && !p.n_glyphs && !p.cached && !p.n_mcells && L.n == 0, id, "a plan without tiles has something to launch");
    else require(L.n >= 1 && L.l[L.n - 1].family == (p.cached ? fr::TL_CACHED : fr::TL_TEXT) && L.l[L.n - 1].grid == p.n_tiles &&
                 L.l[L.n - 1].count == p.n_insts, id, "the list does not end in the plan's text kernel over its tiles");
    require(L.n == (p.n_glyphs ? 1u : 0u) + (p.cached ? 1u : 0u) + (p.n_tiles ? 1u : 0u), id, "launch count");
    require(!p.n_insts == !p.n_glyphs && (!p.cached || (p.n_mcells && p.n_mtiles >= p.n_mcells && p.n_glyphs)), id, "instances, glyphs and mask cells disagree");
    for (uint32_t i = 0; i < L.n; ++i) {
        char name[96];
        fr::text_launch_name(L.l[i], name, sizeof name);
        require(name[0] != 0 && L.l[i].grid != 0, id, "a launch without a kernel or without workgroups");
        require(i == 0 || L.l[i - 1].family < L.l[i].family, id, "launches out of stream order");
    }
}

const char *const FAMILY[4] = {"prepare", "mask", "text", "cached"};
enum Mode { TABLES, OVER, LAUNCHES };

struct Outcome { bool ok; uint64_t hash; int blend; };   // (over) of one form of a case: the hash leaves the blend value out

template <class PLACE>
Outcome run_form(const Case &c, const char *form, Mode mode = TABLES)
{
    const std::string id = std::string(c.name) + "/" + form;
    std::vector<PLACE> places;
    for (const Place &p : c.places) places.push_back(convert(p, c.scale, (const PLACE *)nullptr));
    fr::TextPlanIn in{};
    in.runs = c.null_runs ? nullptr : c.runs.data();
    in.n_runs = (uint32_t)c.runs.size();
    in.n_places = (uint32_t)places.size();
    in.place_rgba = c.colours.empty() ? nullptr : c.colours.data();
    in.run_clear_rgba = c.clears.empty() ? nullptr : c.clears.data();
    in.rgba = c.rgba;
    in.flags = c.flags;
    in.boxes = c.no_boxes ? nullptr : &BOXES[0][0];
    in.glyph_seg_start = SEG_START;
    in.n_glyphs = 6;
    fr::TextPlanTables<PLACE> t;
    clear_error();
    const int rc = fr::text_plan_tables(in, c.null_places ? nullptr : places.data(), t);
    if (rc != FR_OK) {
        printf("%s error %d: %s\n", id.c_str(), rc, last_error());
        return Outcome{false, 0, 0};
    }
    properties(id, c, t);
    // the launches: as fr_api.hip makes them, FR_TEXT_CACHE tables included where the form has them and some cell exists
    fr::TextCacheTables cache;
    if constexpr (!std::is_same<PLACE, fr_glyph_place_affine>::value) {
        if (c.flags & FR_TEXT_CACHE) require(fr::text_cache_tables(in, places.data(), t, cache) == FR_OK, id, "text_cache_tables failed");
    }
    const fr_raster_params params{FR_COVERAGE_U8, c.samples, FR_SAMPLE_CENTER, 0};
    const fr::TextPlan plan = fr::text_plan_of(in, params, t, cache.cells.empty() ? nullptr : &cache);
    fr::TextLaunchList L;
    fr::text_launches(plan, L);
    launch_properties(id, plan, L);
    if (mode == LAUNCHES) {
        printf("%s/launches %u\n", id.c_str(), L.n);
        for (uint32_t i = 0; i < L.n; ++i) {
            char name[96];
            fr::text_launch_name(L.l[i], name, sizeof name);
            printf("%s/launch%u %s %s grid %u count %u\n", id.c_str(), i, FAMILY[L.l[i].family], name, L.l[i].grid, L.l[i].count);
        }
        return Outcome{true, 0, t.blend};
    }
    Fnv f;
    f.vec(t.runs); f.vec(t.tiles); f.vec(t.insts); f.vec(t.list); f.vec(t.glyphs);
    f.u64(t.pixels); f.u64(t.need_cols); f.u64(t.need_rows);
    if (mode == OVER) {
        printf("%s %016llx insts %zu blend %d\n", id.c_str(), (unsigned long long)f.h, t.insts.size(), t.blend);
        return Outcome{true, f.h, t.blend};
    }
    f.u64((uint64_t)t.blend);
    printf("%s %016llx runs %zu tiles %zu insts %zu pairs %zu glyphs %zu\n", id.c_str(), (unsigned long long)f.h, t.runs.size(), t.tiles.size(),
           t.insts.size(), t.list.size(), t.glyphs.size());
    return Outcome{true, f.h, t.blend};
}

// (over) the case as given, then the same with FR_TEXT_OVER under the name <case>_over: equal tables, blend 1 -> 2, 0 -> 0
template <class PLACE>
void run_over_form(const Case &c, const char *form)
{
    const Outcome plain = run_form<PLACE>(c, form, OVER);
    Case o = c;
    const std::string name = std::string(c.name) + "_over";
    o.name = name.c_str();
    o.flags |= FR_TEXT_OVER;
    const Outcome with = run_form<PLACE>(o, form, OVER);
    const std::string id = name + "/" + form;
    require(plain.ok && with.ok, id, "an FR_TEXT_OVER case failed to build");
    require(plain.hash == with.hash, id, "FR_TEXT_OVER changed a table");
    require(with.blend == (plain.blend ? 2 : 0), id, "blend is not 2 for translucent colours and 0 for opaque ones under FR_TEXT_OVER");
}

void run_case(const Case &c, Mode mode = TABLES)
{
    if (c.forms & PLAIN) run_form<fr_glyph_place>(c, "plain", mode);
    if (c.forms & EX) run_form<fr_glyph_place_ex>(c, "ex", mode);
    if (c.forms & AFFINE) run_form<fr_glyph_place_affine>(c, "affine", mode);
}

// (launches) text_launch_name over a box of keys around the valid ones: a line per key that gets a name, then the counts.
// The composites have neither a form nor FILL and the mask kernels no form, colour or BLEND: those stay 0 in their keys
void sweep_names()
{
    unsigned keys = 0, named = 0;
    for (int family = fr::TL_MASK; family <= fr::TL_CACHED; ++family)
        for (int form = 0; form <= (family == fr::TL_TEXT ? 3 : 0); ++form)
            for (int colour = (family == fr::TL_MASK ? 0 : -1); colour <= (family == fr::TL_MASK ? 0 : 5); ++colour)
                for (int n = 0; n <= 5; ++n)
                    for (int fill = (family == fr::TL_CACHED ? 0 : -1); fill <= (family == fr::TL_CACHED ? 0 : 2); ++fill)
                        for (int blend = (family == fr::TL_MASK ? 0 : -1); blend <= (family == fr::TL_MASK ? 0 : 3); ++blend) {
                            const fr::TextLaunch e{(fr::TextFamily)family, (fr::TextForm)form, colour, n, fill, blend, 1u, 1u};
                            char name[96];
                            fr::text_launch_name(e, name, sizeof name);
                            ++keys;
                            if (!name[0]) continue;
                            ++named;
                            printf("name/%s/form%d/colour%d/n%d/fill%d/blend%d %s\n", FAMILY[family], form, colour, n, fill, blend, name);
                        }
    printf("name/swept keys %u named %u\n", keys, named);
}

std::vector<uint8_t> colours(size_t n, uint8_t alpha_of_second)
{
    std::vector<uint8_t> v;
    for (size_t k = 0; k < n; ++k) {
        v.push_back((uint8_t)(225 - 40 * k)); v.push_back((uint8_t)(105 + 7 * k)); v.push_back((uint8_t)(180 + 3 * k));
        v.push_back(k == 1 ? alpha_of_second : 255);
    }
    return v;
}

}  // namespace

int main(int argc, char **argv)
{
    const bool over = argc > 1 && !strcmp(argv[1], "over"), launches = argc > 1 && !strcmp(argv[1], "launches");
    const float S = 0.5f;
    const std::vector<Place> three = {at(0, 5 * 64, 20 * 64), at(1, 20 * 64, 25 * 64), at(2, 10 * 64, 22 * 64)};
    auto R = [&](uint32_t count) { return std::vector<fr_text_run>{run(0, count, 40, 30, 3, 5, S)}; };   // one run of `count` placements
    const std::vector<fr_text_run> one = R(3);
    const std::vector<uint8_t> clear1 = {10, 20, 30, 255};
    std::vector<Case> cases;
    auto add = [&](const char *name, int forms, std::vector<fr_text_run> runs, std::vector<Place> places) -> Case & {
        cases.push_back(Case{name, forms, false, 0u, S, std::move(runs), std::move(places), {}, {}});
        return cases.back();
    };
    auto rgba = [&](Case &c, uint32_t flags, uint8_t alpha, bool clears = true) {
        c.rgba = true; c.flags = flags; c.colours = colours(c.places.size(), alpha);
        for (size_t r = 0; clears && r < c.runs.size(); ++r)
            for (int k = 0; k < 4; ++k) c.clears.push_back((uint8_t)(10 * (k + 1) + r));
    };
    if (over) {
        rgba(add("translucent", ALL, one, three), 0u, 128);
        rgba(add("opaque", ALL, one, three), 0u, 255);
        rgba(add("alpha_zero_srgb_bgra", ALL, one, three), FR_TEXT_SRGB | FR_TEXT_BGRA, 0);
        rgba(add("load_srgb", ALL, {run(0, 3, 200, 40, 7, 9, S)}, three), FR_TEXT_LOAD | FR_TEXT_SRGB, 3, false);
        rgba(add("load_opaque", ALL, {run(0, 3, 200, 40, 0, 0, S)}, three), FR_TEXT_LOAD, 255, false);
        // the translucent colour belongs to a placement that is clipped away: blend looks at every placement, as without the flag
        rgba(add("translucent_clipped_away", ALL, R(3), {at(0, 5 * 64, 20 * 64), at(1, 1000 * 64, 25 * 64), at(2, 10 * 64, 22 * 64)}), 0u, 200);
        for (const Case &c : cases) {
            if (c.forms & PLAIN) run_over_form<fr_glyph_place>(c, "plain");
            if (c.forms & EX) run_over_form<fr_glyph_place_ex>(c, "ex");
            if (c.forms & AFFINE) run_over_form<fr_glyph_place_affine>(c, "affine");
        }
        return exit_status();
    }
    if (launches) {
        // cases of the other two lists with the flags and sample counts that choose an instance, and the three plans whose
        // lists are short: all placements clipped away with and without FR_TEXT_LOAD, and no run at all
        const std::vector<Place> away = {at(0, 1000 * 64, 20 * 64), at(2, 10 * 64, -400 * 64)};
        add("coverage", ALL, one, three);
        add("coverage_fill_n1", ALL, one, three).flags = FR_FILL_CONSISTENT;
        cases.back().samples = 1;
        add("coverage_cached", PLAIN | EX, one, three).flags = FR_TEXT_CACHE;
        rgba(add("rgba_translucent_over_n2", ALL, one, three), FR_TEXT_OVER | FR_FILL_CONSISTENT, 128);
        cases.back().samples = 2;
        rgba(add("rgba_srgb_bgra", ALL, one, three), FR_TEXT_SRGB | FR_TEXT_BGRA, 255);
        rgba(add("rgba_load", ALL, {run(0, 3, 200, 40, 0, 0, S)}, three), FR_TEXT_LOAD, 255, false);
        rgba(add("rgba_load_srgb_translucent_cached", PLAIN | EX, {run(0, 3, 200, 40, 7, 9, S)}, three), FR_TEXT_LOAD | FR_TEXT_SRGB | FR_TEXT_CACHE | FR_FILL_CONSISTENT, 3, false);
        rgba(add("two_runs_cached", PLAIN | EX, {run(0, 2, 40, 30, 0, 0, S), run(2, 3, 70, 20, 40, 0, S)},
                 {at(0, 5 * 64, 20 * 64), at(1, 20 * 64, 25 * 64), at(2, 10 * 64, 12 * 64), at(4, 30 * 64, 18 * 64), at(1, 60 * 64, 15 * 64)}),
             FR_TEXT_CACHE, 255);
        rgba(add("affine_general", AFFINE, {run(0, 3, 130, 50, 0, 0, S)},
                 {mat(4, 20 * 64 + 3, 45 * 64 + 60, 0.4f, 0.3f, -0.2f, 0.6f), mat(2, 90 * 64, 30 * 64, -0.7f, 0.45f, 0.15f, 0.9f), mat(1, 5 * 64, 5 * 64, 3.0f, -1.0f, 2.0f, 0.125f)}),
             FR_TEXT_SRGB, 200);
        rgba(add("load_all_clipped_away", ALL, R(2), away), FR_TEXT_LOAD, 128, false);
        add("tiles_but_no_instance", ALL, R(2), away);
        add("tiles_but_no_instance_cached", PLAIN | EX, R(2), away).flags = FR_TEXT_CACHE;
        add("no_runs", ALL, {}, three);
        for (const Case &c : cases) run_case(c, LAUNCHES);
        sweep_names();
        return exit_status();
    }
    add("coverage", ALL, one, three);
    rgba(add("rgba_translucent", ALL, one, three), 0u, 128);
    rgba(add("rgba_srgb_bgra", ALL, one, three), FR_TEXT_SRGB | FR_TEXT_BGRA, 255);
    rgba(add("rgba_load", ALL, {run(0, 3, 200, 40, 0, 0, S)}, three), FR_TEXT_LOAD, 255, false);
    rgba(add("rgba_load_srgb_translucent", ALL, {run(0, 3, 200, 40, 7, 9, S)}, three), FR_TEXT_LOAD | FR_TEXT_SRGB, 3, false);
    add("pen_fx", ALL, R(2), {at(0, 5 * 64 + 17, 20 * 64), at(1, 20 * 64 + 63, 25 * 64)});
    add("pen_fy", EX | AFFINE, R(2), {at(0, 5 * 64, 20 * 64 + 33), at(1, 20 * 64 + 1, 25 * 64 + 63)});
    add("pen_negative", ALL, R(3), {at(4, -100, 20 * 64), at(2, 3 * 64, -70), at(0, -1, -1 + 12 * 64)});
    add("clipped_away", ALL, R(4), {at(0, 1000 * 64, 20 * 64), at(1, 20 * 64, 25 * 64), at(2, 10 * 64, -400 * 64), at(0, -11 * 64, 10 * 64)});
    add("clipped_each_side", ALL, {run(0, 5, 30, 30, 0, 0, S)},
        {at(1, -3 * 64, 15 * 64), at(1, 27 * 64, 15 * 64), at(1, 10 * 64, 3 * 64), at(1, 10 * 64, 33 * 64), at(4, -10 * 64, 40 * 64)});
    add("no_segments", ALL, R(3), {at(3, 5 * 64, 20 * 64), at(1, 20 * 64, 25 * 64), at(3, 6 * 64, 20 * 64)});
    add("zero_width_run", ALL, {run(0, 2, 0, 20, 100, 0, S), run(1, 2, 40, 30, 0, 0, S), run(0, 3, 20, 0, 0, 100, S)}, three);
    add("run_65x17", ALL, {run(0, 3, 65, 17, 1, 2, S)}, {at(1, 2 * 64, 12 * 64), at(4, 30 * 64, 30 * 64), at(0, 56 * 64 + 5, 16 * 64)});
    rgba(add("two_runs", ALL, {run(0, 2, 40, 30, 0, 0, S), run(2, 3, 70, 20, 40, 0, S)},
             {at(0, 5 * 64, 20 * 64), at(1, 20 * 64, 25 * 64), at(2, 10 * 64, 12 * 64), at(4, 30 * 64, 18 * 64), at(1, 60 * 64, 15 * 64)}),
         0u, 255);
    add("two_runs_shared_places", ALL, {run(0, 3, 40, 30, 0, 40, S), run(1, 2, 64, 16, 0, 0, S)}, three);
    add("no_runs", ALL, {}, three);
    add("ex_own_scale", EX | AFFINE, R(3), {at(0, 5 * 64, 20 * 64, 0.75f), at(1, 20 * 64, 25 * 64), at(2, 10 * 64, 22 * 64, 0.3f)});
    add("ex_slant", EX | AFFINE, R(4), {at(0, 5 * 64, 20 * 64, 0.0f, 0.25f), at(1, 20 * 64 + 9, 25 * 64 + 7, 0.75f, -0.3f), at(2, 10 * 64, 22 * 64, 0.0f, 4.0f),
                                       at(2, 30 * 64, 22 * 64, 0.0f, -4.0f)});
    add("affine_identity", AFFINE, {run(0, 2, 40, 30, 3, 5, 1.0f)}, {mat(0, 5 * 64, 26 * 64, 1, 0, 0, 1), mat(1, 20 * 64 + 5, 25 * 64 + 9, 1, 0, 0, 1)});
    add("affine_quarter_turn", AFFINE, R(2), {mat(0, 25 * 64, 20 * 64, 0, -S, S, 0), mat(2, 30 * 64 + 31, 4 * 64 + 1, 0, S, -S, 0)});
    add("affine_mirror", AFFINE, R(2), {mat(0, 25 * 64, 20 * 64, -S, 0, 0, S), mat(2, 20 * 64, 4 * 64, S, 0, 0, -S)});
    rgba(add("affine_general", AFFINE, {run(0, 3, 130, 50, 0, 0, S)},
             {mat(4, 20 * 64 + 3, 45 * 64 + 60, 0.4f, 0.3f, -0.2f, 0.6f), mat(2, 90 * 64, 30 * 64, -0.7f, 0.45f, 0.15f, 0.9f), mat(1, 5 * 64, 5 * 64, 3.0f, -1.0f, 2.0f, 0.125f)}),
         FR_TEXT_SRGB, 200);

    // one failing case per message
    add("err_places_null", ALL, one, three).null_places = true;
    add("err_runs_null", ALL, one, three).null_runs = true;
    { Case &c = add("err_place_rgba_null", ALL, one, three); c.rgba = true; c.clears = clear1; }
    { Case &c = add("err_run_clear_rgba_null", ALL, one, three); c.rgba = true; c.colours = colours(3, 255); }
    add("err_no_boxes", ALL, one, three).no_boxes = true;
    add("err_run_places_range", ALL, {run(2, 2, 40, 30, 0, 0, S)}, three);
    add("err_run_scale_zero", ALL, {run(0, 3, 40, 30, 0, 0, 0.0f)}, three);
    add("err_run_scale_small", ALL, {run(0, 3, 40, 30, 0, 0, 4.0e-7f)}, three);
    add("err_run_too_large", ALL, {run(0, 3, 65536, 30, 0, 0, S)}, three);
    add("err_glyph_index", ALL, R(2), {at(0, 0, 0), at(6, 0, 0)});
    add("err_pen_x_range", ALL, R(1), {at(0, 0x7fffffff, 0)});
    add("err_pen_y_range", ALL, R(1), {at(0, 0, 0x7fffffff)});
    add("err_matrix_singular", AFFINE, R(1), {mat(0, 0, 0, 1, 2, 2, 4)});
    add("err_matrix_large", AFFINE, R(1), {mat(0, 0, 0, 2097152.0f, 0, 0, 1)});
    add("err_matrix_inverse_large", AFFINE, R(1), {mat(0, 0, 0, 4.0e-7f, 0, 0, 1)});
    add("err_place_scale_negative", EX, R(1), {at(0, 0, 0, -1.0f)});
    add("err_place_scale_large", EX, R(1), {at(0, 0, 0, 2097152.0f)});
    add("err_place_slant_infinite", EX, R(1), {at(0, 0, 0, 0.0f, INFINITY)});
    add("err_place_slant_large", EX, R(1), {at(0, 0, 0, 0.0f, 4.5f)});
    add("err_too_many_tiles", ALL, std::vector<fr_text_run>(600, run(0, 0, 65535, 65535, 0, 0, S)), {});
    add("err_runs_overlap", ALL, {run(0, 1, 40, 30, 0, 0, S), run(1, 1, 0, 30, 10, 10, S), run(1, 2, 40, 30, 39, 29, S)}, three);
    add("err_cell_too_large", ALL, {run(0, 1, 40, 30, 0, 0, 1024.0f)}, {at(4, 0, 0)}).scale = 1024.0f;
    // the order of the checks: the first of several faults wins
    add("err_order_run_before_place", ALL, {run(0, 1, 40, 30, 0, 0, S), run(0, 2, 70000, 30, 0, 100, S)}, {at(0, 0, 0), at(9, 0, 0)});
    add("err_order_glyph_before_pen", ALL, R(1), {at(9, 0x7fffffff, 0)});
    add("err_order_pen_before_matrix", EX | AFFINE, R(1), {Place{0, 0x7fffffff, 0, -1.0f, 0.0f, {1, 2, 2, 4}}});

    for (const Case &c : cases) run_case(c);
    return exit_status();
}

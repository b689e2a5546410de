// fr_text_plan.hpp — the host tables of a text plan, resolved from the caller's placements and runs (fr_text_plan.cpp).
// Plain C++: no HIP, no fr_ctx, no fr_plan.  fr_api.hip checks the context and the raster parameters, calls
// text_plan_tables, uploads what it returns and launches the kernels; host/text_plan_selftest.cpp runs it on the CPU.
#pragma once
#include "../../include/fr_raster.h"
#include "fr_text_tables.hpp"

#include <vector>

namespace fr {

struct TextPlanIn {                    // everything the tables depend on besides the placements
    const fr_text_run *runs;
    uint32_t n_runs, n_places;
    const uint8_t *place_rgba;         // rgba: 4 bytes per placement
    const uint8_t *run_clear_rgba;     // rgba without FR_TEXT_LOAD: 4 bytes per run
    bool rgba;                         // an RGBA plan (the colours above are read); else coverage / mask bytes
    uint32_t flags;                    // FR_TEXT_SRGB, FR_TEXT_BGRA, FR_TEXT_LOAD, FR_TEXT_OVER (other bits are not looked at)
    const int16_t *boxes;              // the glyph set's Glyph.box per glyph (x_min, y_min, x_max, y_max); NULL: never set
    const uint32_t *glyph_seg_start;   // its n_glyphs + 1 segment offsets
    uint32_t n_glyphs;
};

// the instance record of a placement form
template <class PLACE> struct TextInstOf;
template <> struct TextInstOf<fr_glyph_place> { using type = TextInst; };
template <> struct TextInstOf<fr_glyph_place_ex> { using type = TextInstEx; };
template <> struct TextInstOf<fr_glyph_place_affine> { using type = TextInstAffine; };

template <class PLACE>
struct TextPlanTables {
    std::vector<TextRun> runs;
    std::vector<TextTile> tiles;       // every 64 x 16 tile of every run; under FR_TEXT_LOAD only those some instance meets
    std::vector<typename TextInstOf<PLACE>::type> insts;   // the placements that survive clipping, in placement order
    std::vector<uint32_t> list;        // the tiles' instance lists (TextTile::lbeg, lend), each in placement order
    std::vector<uint32_t> glyphs;      // the distinct glyphs of insts, ascending
    uint64_t pixels = 0, need_cols = 0, need_rows = 0;
    int blend = 0;                     // (rgba) 0: every placement colour is opaque; else 1, or 2 under FR_TEXT_OVER
};

// PLACE: fr_glyph_place, fr_glyph_place_ex or fr_glyph_place_affine.  FR_OK, or the code include/fr_raster.h names with
// its message left through fr::set_error.
template <class PLACE>
int text_plan_tables(const TextPlanIn &in, const PLACE *places, TextPlanTables<PLACE> &out);

// ---- FR_TEXT_CACHE: one mask cell per key, filled once per render and read by every instance of the key ----------------
struct TextCacheTables {
    std::vector<TextMaskCell> cells;   // one per distinct key among the surviving instances, in order of first use
    std::vector<TextMaskTile> tiles;   // every 64 x 16 tile of every cell, cell by cell
    std::vector<TextCachedInst> insts; // one per instance of TextPlanTables::insts, in its order (the tiles' lists name both alike)
    uint64_t elems = 0;                // the mask store: the sum of cw * ch over the cells, uint16_t each
};

constexpr uint64_t TEXT_CACHE_MAX_ELEMS = (uint64_t)1 << 31;

// PLACE: fr_glyph_place (key: glyph, pen_x64 mod 64, the bits of the run's scale) or fr_glyph_place_ex (key: glyph, pen_x64
// mod 64, pen_y64 mod 64, the bits of the effective scale and of the slant).  `in`, `places` and `t` are what
// text_plan_tables took and returned.  FR_OK, or FR_E_UNSUPPORTED (message through fr::set_error) when the cells hold
// more than TEXT_CACHE_MAX_ELEMS elements: decided before any tile is listed, so the caller has nothing to allocate.
template <class PLACE>
int text_cache_tables(const TextPlanIn &in, const PLACE *places, const TextPlanTables<PLACE> &t, TextCacheTables &out);

}  // namespace fr

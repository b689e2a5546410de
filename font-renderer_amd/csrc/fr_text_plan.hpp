// fr_text_plan.hpp — the host tables of a text plan, resolved from the caller's placements and runs, and the launches of
// one render as a list (fr_text_plan.cpp).  Plain C++: no HIP, no fr_ctx, no fr_plan.  fr_api.hip checks the context and
// the raster parameters, calls text_plan_tables, uploads what it returns, and walks text_launches twice: to launch
// (text_launch) and to name (fr_plan_describe); host/text_plan_selftest.cpp runs all of it on the CPU.  A launch of the
// list names its kernel instance completely: the kernel units only look it up (pick, fr_device.hpp).
#pragma once
#include "../../include/fr_raster.h"
#include "fr_text_tables.hpp"

#include <cstddef>
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
    std::vector<TextMaskCellAffine> acells;   // the same for fr_glyph_place_affine placements: a plan fills one of the two
    std::vector<TextMaskTile> tiles;   // every 64 x 16 tile of every cell, cell by cell
    std::vector<TextCachedInst> insts; // one per instance of TextPlanTables::insts, in its order (the tiles' lists name both alike)
    uint64_t elems = 0;                // the mask store: the sum of cw * ch over the cells, uint16_t each
    size_t n_cells() const { return cells.size() + acells.size(); }
};

constexpr uint64_t TEXT_CACHE_MAX_ELEMS = (uint64_t)1 << 31;

// PLACE: fr_glyph_place (key: glyph, pen_x64 mod 64, the bits of the run's scale), fr_glyph_place_ex (key: glyph, pen_x64
// mod 64, pen_y64 mod 64, the bits of the effective scale and of the slant) or, for FR_TEXT_CACHE_AFFINE,
// fr_glyph_place_affine (key: glyph, pen_x64 mod 64, pen_y64 mod 64, the bits of m[0..3]; its cells are `acells`).  `in`,
// `places` and `t` are what
// text_plan_tables took and returned.  FR_OK, or FR_E_UNSUPPORTED (message through fr::set_error) when the cells hold
// more than TEXT_CACHE_MAX_ELEMS elements: decided before any tile is listed, so the caller has nothing to allocate.
template <class PLACE>
int text_cache_tables(const TextPlanIn &in, const PLACE *places, const TextPlanTables<PLACE> &t, TextCacheTables &out);

// ---- the launches of one render ----------------------------------------------------------------------------------------
// the placement form: fr_glyph_place (TextInst, the text_* kernels), fr_glyph_place_ex (TextInstEx, text_place_*) or
// fr_glyph_place_affine (TextInstAffine, the text_affine_* kernels of fr_text_affine.hip)
enum TextForm : uint8_t { TEXT_PLAIN, TEXT_EX, TEXT_AFFINE };
constexpr TextForm text_form_of(const fr_glyph_place *) { return TEXT_PLAIN; }
constexpr TextForm text_form_of(const fr_glyph_place_ex *) { return TEXT_EX; }
constexpr TextForm text_form_of(const fr_glyph_place_affine *) { return TEXT_AFFINE; }

struct TextPlan {                      // everything the launches of a text plan's render depend on
    TextForm form = TEXT_PLAIN;        // which record the instance table holds and which kernels read it
    bool rgba = false;                 // RGBA pixels; else coverage / mask bytes
    bool srgb = false;                 // (rgba) FR_TEXT_SRGB: blending and resolve in linear light
    bool load = false;                 // (rgba) FR_TEXT_LOAD: the samples start at the output's pixels; occupied tiles only
    bool cached = false;               // FR_TEXT_CACHE / FR_TEXT_CACHE_AFFINE with at least one mask cell: the instance table holds TextCachedInst
    int blend = 0;                     // (rgba) TextPlanTables::blend
    int fill = 0;                      // FR_FILL_CONSISTENT
    int samples = 1;                   // per axis
    uint32_t n_tiles = 0, n_insts = 0, n_glyphs = 0;
    uint32_t n_mcells = 0, n_mtiles = 0;   // (cached) the mask cells and their tiles
};
// the one place that reads a text plan's flag bits for its launches.  `cache`: the tables of text_cache_tables for a plan
// that renders through its mask cells, else NULL
template <class PLACE>
TextPlan text_plan_of(const TextPlanIn &in, const fr_raster_params &params, const TextPlanTables<PLACE> &t, const TextCacheTables *cache);

enum TextFamily : uint8_t { TL_PREPARE, TL_MASK, TL_TEXT, TL_CACHED };
struct TextLaunch {
    TextFamily family;                 // prepare_kernel, glyph_mask_kernel (glyph_mask_affine_kernel), a text kernel of `form`, a cached composite
    TextForm form;                     // (text; mask: TEXT_AFFINE picks glyph_mask_affine_kernel and its cell record)
    int colour;                        // (text, cached) 0 coverage, 1 rgba, 2 srgb, 3 rgba load, 4 srgb load
    int n, fill, blend;                // the template arguments N, FILL, BLEND: the coverage kernels have no BLEND (0), the
                                       // composites no FILL (0: the fill rule acts only where masks are made)
    uint32_t grid;                     // workgroups: glyphs, mask tiles, run tiles
    uint32_t count;                    // what fr_plan_describe prints beside the name: glyphs, mask cells, instances
};
struct TextLaunchList {
    TextLaunch l[3];                   // in stream order: prepare, mask (cached plans), text or composite
    uint32_t n = 0;
};
void text_launches(const TextPlan &p, TextLaunchList &out);
// the kernel of a launch as rocprofv3 names it, into name[cap]; "" for arguments the kernels have no instance of, which
// end the launch in hipErrorInvalidValue: N outside {1, 2, 4}, FILL outside {0, 1}, BLEND outside {0, 1, 2}, coverage with BLEND != 0
void text_launch_name(const TextLaunch &e, char *name, size_t cap);

}  // namespace fr

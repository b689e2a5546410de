// fr_text.hpp — what a text kernel reads (the tables of fr_text_tables.hpp, on the device) and how fr_api.hip launches it
#pragma once
#include "fr_device.hpp"
#include "fr_text_tables.hpp"

namespace fr {

template <class INST>
struct TextTables {        // what a text kernel reads, for either placement form
    const TextTile *tiles;
    const TextRun *runs;
    const INST *insts;
    const uint32_t *list;
    const Rec *recs;
    const uint32_t *rec_count;
    uint8_t *out;          // bytes, or the RGBA pixels (4-byte aligned) of the colour kernels
    uint64_t out_stride;   // elements
    int32_t phase_center;
};
struct TextArgs : TextTables<TextInst> {};         // fr_glyph_place placements: the text_*_kernel instances
struct TextPlaceArgs : TextTables<TextInstEx> {};  // fr_glyph_place_ex placements: the text_place_*_kernel instances
struct TextAffineArgs : TextTables<TextInstAffine> {};  // fr_glyph_place_affine placements: the text_affine_*_kernel instances

// Launches the instance of a plan: n in {1, 2, 4}; rgba = 0: coverage / mask bytes (text_kernel; blend, srgb and load are
// then ignored); else blend = 0 when every placement colour of the plan is opaque (A = 255), srgb for FR_TEXT_SRGB plans
// (blending and resolve in linear light), load for FR_TEXT_LOAD plans (the samples start at the output's pixels; n_tiles
// then counts only the tiles with a non-empty instance list).  n_tiles = 0: only name the instance (as rocprofv3 names
// it) into name[name_cap].  ARGS: TextArgs or TextPlaceArgs (fr_text.hip), or TextAffineArgs (fr_text_affine.hip).
template <class ARGS>
hipError_t launch_text(const ARGS &a, int n, int fill, int rgba, int blend, int srgb, int load, uint32_t n_tiles, hipStream_t stream,
                       char *name = nullptr, size_t name_cap = 0);

// ---- FR_TEXT_CACHE plans (fr_text_cached.hip) ---------------------------------------------------------------------------
struct TextMaskArgs {      // what glyph_mask_kernel reads and writes
    const TextMaskTile *tiles;
    const TextMaskCell *cells;
    const Rec *recs;
    const uint32_t *rec_count;
    uint16_t *masks;       // the mask store
    int32_t phase_center;
};
struct TextCachedArgs : TextTables<TextCachedInst> {   // the text_cached_*_kernel instances (recs and rec_count are not read)
    const uint16_t *masks;
};

// Fills every mask cell: glyph_mask_kernel<n, fill> over n_tiles mask tiles.  n_tiles = 0: only names the instance.
hipError_t launch_glyph_mask(const TextMaskArgs &a, int n, int fill, uint32_t n_tiles, hipStream_t stream, char *name = nullptr,
                             size_t name_cap = 0);
// The composite of a cached plan over n_tiles run tiles; the parameters as launch_text's, without the fill rule (it acts
// only where masks are made).  n_tiles = 0: only names the instance.
hipError_t launch_text_cached(const TextCachedArgs &a, int n, int rgba, int blend, int srgb, int load, uint32_t n_tiles,
                              hipStream_t stream, char *name = nullptr, size_t name_cap = 0);

}  // namespace fr

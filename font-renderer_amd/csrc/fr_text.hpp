// fr_text.hpp — what a text kernel reads (the tables of fr_text_tables.hpp, on the device) and how fr_api_plan.hip launches it
#pragma once
#include "fr_device.hpp"
#include "fr_text_plan.hpp"
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

// The launch of a text plan's launch list (fr_text_plan.hpp) that runs a text kernel over e.grid tiles: e names the
// instance (colour family, N, FILL, BLEND), the argument type says which form's.  TextArgs and TextPlaceArgs:
// fr_text.hip; TextAffineArgs: fr_text_affine.hip.  hipErrorInvalidValue for arguments the kernels have no instance of.
hipError_t launch_text(const TextLaunch &e, const TextArgs &a, hipStream_t stream);
hipError_t launch_text(const TextLaunch &e, const TextPlaceArgs &a, hipStream_t stream);
hipError_t launch_text(const TextLaunch &e, const TextAffineArgs &a, hipStream_t stream);

// one workgroup of TEXT_WAVES waves per tile
template <class ARGS>
inline hipError_t launch_tiles(void (*kernel)(ARGS), uint32_t n_tiles, hipStream_t stream, const ARGS &a)
{
    hipLaunchKernelGGL(kernel, dim3(n_tiles), dim3(64 * TEXT_WAVES), 0, stream, a);
    return hipGetLastError();
}
// the look-up of both units: of(FAM, FILL, BLEND, N) is the unit's kernel for ARGS (the coverage kernels have no BLEND)
template <class ARGS, class OF>
inline hipError_t launch_text_instance(const TextLaunch &e, const ARGS &a, hipStream_t stream, OF of)
{
    const int key[] = {e.colour, e.fill, e.blend, e.n};
    return pick(key, [&](auto FAM, auto FILL, auto BLEND, auto N) {
        if constexpr (decltype(FAM)::value == 0 && decltype(BLEND)::value != 0) return hipErrorInvalidValue;
        else return launch_tiles<ARGS>(of(FAM, FILL, BLEND, N), e.grid, stream, a);
    }, Among<0, 1, 2, 3, 4>{}, Among<0, 1>{}, Among<0, 1, 2>{}, Among<1, 2, 4>{});
}

// ---- FR_TEXT_CACHE and FR_TEXT_CACHE_AFFINE plans (fr_text_cached.hip) --------------------------------------------------
struct TextMaskArgs {      // what glyph_mask_kernel and glyph_mask_affine_kernel read and write
    const TextMaskTile *tiles;
    const void *cells;     // TextMaskCell; glyph_mask_affine_kernel: TextMaskCellAffine (as TextView::insts, the form says which)
    const Rec *recs;
    const uint32_t *rec_count;
    uint16_t *masks;       // the mask store
    int32_t phase_center;
};
struct TextCachedArgs : TextTables<TextCachedInst> {   // the text_cached_*_kernel instances (recs and rec_count are not read)
    const uint16_t *masks;
};

// Fills every mask cell: glyph_mask_kernel<e.n, e.fill>, or glyph_mask_affine_kernel<e.n, e.fill> when e.form is TEXT_AFFINE,
// over e.grid mask tiles.  hipErrorInvalidValue for a form, n or fill the kernels have no instance of.
hipError_t launch_glyph_mask(const TextLaunch &e, const TextMaskArgs &a, hipStream_t stream);
// The composite of a cached plan over e.grid run tiles: the instance of (e.colour, e.n, e.blend); no fill rule (it acts
// only where masks are made).
hipError_t launch_text_cached(const TextLaunch &e, const TextCachedArgs &a, hipStream_t stream);

}  // namespace fr

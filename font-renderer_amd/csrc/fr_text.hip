// fr_text.hip — text runs (include/fr_raster.h, DESIGN.md sections 4.7 and 5): the union over overlapping glyph
// instances of the non-zero test, per sample, composited into each run's image in one pass.
//
// One workgroup of four waves takes one TILE of a run: 64 image columns x 16 image rows; a wave takes every fourth row
// of it, one pixel per lane.  The plan lists, once on the host, the instances whose (clipped) cells meet each tile.  For
// one row and one instance every ray height cy is the same in all lanes, so the root of each record — the reference's
// own arithmetic (rec_cross, fr_device.hpp) — is wave-uniform and only the crossing test !(xx < cx) is per lane: n^2
// winding counters per lane, reduced to an n^2-bit mask (winding != 0, fr_text_mask_kernel.inc).  The records are the
// stand-alone ones of prepare_kernel (fr_prepare.hip), rebuilt from the glyph points into plan-owned memory before every
// render, so a glyph of any size takes this path.  A wave's row leaves as consecutive bytes, stored non-temporally.
//
// Two bodies serve every instance, each written once.  fr_text_cover_kernel.inc: coverage / mask bytes, the masks ORed
// over the instances whose cell contains the pixel.  fr_text_colour_kernel.inc: RGBA pixels, the instances' colours
// applied to the lane's n^2 samples in placement order.  Both take the placement form from the instance type (PLACE):
// TextInst of fr_glyph_place, or TextInstEx of fr_glyph_place_ex with its own scale, slant and 1/64-pixel baseline, which
// changes only the map from a sample to the glyph's font units (fr_text_mask_kernel.inc).  The two placement forms stay
// separate instances because the wider record measured 0.7-1.5 % slower on fr_glyph_place plans.
// A third form, TextInstAffine of fr_glyph_place_affine (a 2 x 2 matrix: every lane at its own ray height), uses the same
// two bodies with a mask evaluation of its own; its instances live in fr_text_affine.hip.
// The ten __global__ templates at the end only set the parameters of a body.  Some include it, some call it through
// colour_rows; which, is decided by measurement and explained there.
#include "fr_text.hpp"
#include "fr_text_colour.hpp"
#include "fr_srgb.hpp"
#include "fr_wave.hpp"

#include <type_traits>

namespace fr {

// The rows of one tile as RGBA pixels, one dword per lane (fr_text_colour_kernel.inc).
// BLEND = 0: every placement colour is opaque, so a sample takes the colour of the last instance that covers it: the
// instances are walked backwards and each adds the samples it takes first; the samples none takes add the start value.
// BLEND = 1: n^2 RGBA8 sample states per lane, blended forwards in placement order (src*A + dst*(255 - A) for R G B,
// alpha replaced by A).  BLEND = 2 (FR_TEXT_OVER with a translucent colour): BLEND = 1 with the alpha updated as a colour
// channel whose source is 255, a' = (255*A + a*(255 - A) + 127) div 255: UNORM carries it in the high half of the G
// channel's blend2 call, sRGB adds one div255_24 (alpha stays linear).  An if constexpr in the per-sample loop, so the
// instances of BLEND 0 and 1 compile from the text they had.  Either way the pixel is (sum over the samples + n^2/2) div
// n^2 per channel.
// SRGB (FR_TEXT_SRGB): the colour channels are blended and resolved in 16-bit linear light, c' = E((D[C] * A + D[c] *
// (255 - A) + 127) div 255) and E((sum of D[c] + n^2/2) div n^2), through the tables of fr_srgb.hpp, copied into LDS once
// per workgroup; the host put the linear values of the placement and clear colours in TextInst::pad / TextRun::pad.
// LOAD (FR_TEXT_LOAD): every sample starts at the pixel already in the output instead of the run's clear colour.  Each
// lane loads its pixel (guarded as the store is) before the instance walk, so the load's latency hides under the
// wave-uniform root evaluations.  With BLEND = 0 a lane whose samples are all untaken holds that pixel exactly (the
// resolve of n^2 equal values; for sRGB E(D[v]) = v), so it skips its store and a row costs only its reads where no
// glyph reaches.  The plan launches only the tiles whose instance list is non-empty (fr_text_plan.cpp): a pixel of any other
// tile is neither read nor written.
template <int N, int FILL, int BLEND, bool SRGB, bool LOAD, class INST>
__device__ __forceinline__ void colour_rows(const TextTables<INST> &a)
{
    constexpr bool PLACE = std::is_same_v<INST, TextInstEx>;
#include "fr_text_colour_kernel.inc"
}

// The instances, under the names that rocprofv3 and fr_plan_describe show: each only sets the parameters of a body.
// A body that reaches its kernel through a function is optimised in another order than one written into the kernel, and
// the compiler then orders a few operands and address bases differently: the same instructions in every loop, yet
// text_kernel<2, 0> and text_rgba_load_kernel<2, 0, 1> measured 0.4-0.9 % slower through a function, reproducibly, and
// text_rgba_kernel<2, 0, *> 0.5-1.1 % faster.  So the coverage kernels and the old form's two LOAD families
// include their body, which compiles to the assembly they had as separate copies; the others call colour_rows.
#define FR_TEXT_GLOBAL __global__ __launch_bounds__(64 * TEXT_WAVES) void
template <int N, int FILL>
FR_TEXT_GLOBAL text_kernel(TextArgs a)
{
    using INST = dependent_t<N, TextInst>;
    constexpr bool PLACE = false;
#include "fr_text_cover_kernel.inc"
}
template <int N, int FILL, int BLEND>
FR_TEXT_GLOBAL text_rgba_kernel(TextArgs a) { colour_rows<N, FILL, BLEND, false, false>(a); }
template <int N, int FILL, int BLEND>
FR_TEXT_GLOBAL text_srgb_kernel(TextArgs a) { colour_rows<N, FILL, BLEND, true, false>(a); }
template <int N, int FILL, int BLEND>
FR_TEXT_GLOBAL text_rgba_load_kernel(TextArgs a)
{
    using INST = dependent_t<N, TextInst>;
    constexpr bool SRGB = false, LOAD = true, PLACE = false;
#include "fr_text_colour_kernel.inc"
}
template <int N, int FILL, int BLEND>
FR_TEXT_GLOBAL text_srgb_load_kernel(TextArgs a)
{
    using INST = dependent_t<N, TextInst>;
    constexpr bool SRGB = true, LOAD = true, PLACE = false;
#include "fr_text_colour_kernel.inc"
}
template <int N, int FILL>
FR_TEXT_GLOBAL text_place_kernel(TextPlaceArgs a)
{
    using INST = dependent_t<N, TextInstEx>;
    constexpr bool PLACE = true;
#include "fr_text_cover_kernel.inc"
}
template <int N, int FILL, int BLEND>
FR_TEXT_GLOBAL text_place_rgba_kernel(TextPlaceArgs a) { colour_rows<N, FILL, BLEND, false, false>(a); }
template <int N, int FILL, int BLEND>
FR_TEXT_GLOBAL text_place_srgb_kernel(TextPlaceArgs a) { colour_rows<N, FILL, BLEND, true, false>(a); }
template <int N, int FILL, int BLEND>
FR_TEXT_GLOBAL text_place_rgba_load_kernel(TextPlaceArgs a) { colour_rows<N, FILL, BLEND, false, true>(a); }
template <int N, int FILL, int BLEND>
FR_TEXT_GLOBAL text_place_srgb_load_kernel(TextPlaceArgs a) { colour_rows<N, FILL, BLEND, true, true>(a); }
#undef FR_TEXT_GLOBAL

namespace {

// FAM (TextLaunch::colour): 0 coverage (its kernels have no BLEND), 1 rgba, 2 srgb, 3 rgba load, 4 srgb load
template <class ARGS, int FAM, int FILL, int BLEND, int N>
constexpr auto text_kernel_of() -> void (*)(ARGS)
{
    constexpr bool PLACE = std::is_same_v<ARGS, TextPlaceArgs>;
    if constexpr (FAM == 0) {
        if constexpr (PLACE) return text_place_kernel<N, FILL>;
        else return text_kernel<N, FILL>;
    } else if constexpr (FAM == 1) {
        if constexpr (PLACE) return text_place_rgba_kernel<N, FILL, BLEND>;
        else return text_rgba_kernel<N, FILL, BLEND>;
    } else if constexpr (FAM == 2) {
        if constexpr (PLACE) return text_place_srgb_kernel<N, FILL, BLEND>;
        else return text_srgb_kernel<N, FILL, BLEND>;
    } else if constexpr (FAM == 3) {
        if constexpr (PLACE) return text_place_rgba_load_kernel<N, FILL, BLEND>;
        else return text_rgba_load_kernel<N, FILL, BLEND>;
    } else {
        if constexpr (PLACE) return text_place_srgb_load_kernel<N, FILL, BLEND>;
        else return text_srgb_load_kernel<N, FILL, BLEND>;
    }
}

}  // namespace

hipError_t launch_text(const TextLaunch &e, const TextArgs &a, hipStream_t stream)
{
    return launch_text_instance(e, a, stream, [](auto FAM, auto FILL, auto BLEND, auto N) { return text_kernel_of<TextArgs, FAM, FILL, BLEND, N>(); });
}
hipError_t launch_text(const TextLaunch &e, const TextPlaceArgs &a, hipStream_t stream)
{
    return launch_text_instance(e, a, stream, [](auto FAM, auto FILL, auto BLEND, auto N) { return text_kernel_of<TextPlaceArgs, FAM, FILL, BLEND, N>(); });
}

}  // namespace fr

// fr_text_affine.hip — text runs of fr_glyph_place_affine placements (include/fr_raster.h, DESIGN.md sections 4.7 and 5):
// every placement carries a 2 x 2 matrix, so text runs rotated, mirrored or along any direction.  The tile walk, the
// colour arithmetic, LOAD, sRGB and the stores are the two row bodies of fr_text.hip, unchanged; only the evaluation of an
// instance's mask differs (fr_text_affine_mask_kernel.inc): a sample row's ray height is no longer the same in all 64
// lanes, so every lane solves every record at its own height, and a wave-uniform cull skips the records whose height
// range the row's samples cannot reach.  A translation unit of its own: the 78 instances compile beside the 156 of
// fr_text.hip, and nothing here can move a register of those.
#include "fr_text.hpp"
#include "fr_text_colour.hpp"
#include "fr_srgb.hpp"
#include "fr_wave.hpp"

#include <type_traits>

namespace fr {

template <int N, int FILL, int BLEND, bool SRGB, bool LOAD>
__device__ __forceinline__ void affine_colour_rows(const TextAffineArgs &a)
{
    using INST = dependent_t<N, TextInstAffine>;
    constexpr bool PLACE = false;                                          // (read only by the other forms' mask text)
#include "fr_text_colour_kernel.inc"
}

#define FR_TEXT_GLOBAL __global__ __launch_bounds__(64 * TEXT_WAVES) void
template <int N, int FILL>
FR_TEXT_GLOBAL text_affine_kernel(TextAffineArgs a)
{
    using INST = dependent_t<N, TextInstAffine>;
    constexpr bool PLACE = false;
#include "fr_text_cover_kernel.inc"
}
template <int N, int FILL, int BLEND>
FR_TEXT_GLOBAL text_affine_rgba_kernel(TextAffineArgs a) { affine_colour_rows<N, FILL, BLEND, false, false>(a); }
template <int N, int FILL, int BLEND>
FR_TEXT_GLOBAL text_affine_srgb_kernel(TextAffineArgs a) { affine_colour_rows<N, FILL, BLEND, true, false>(a); }
template <int N, int FILL, int BLEND>
FR_TEXT_GLOBAL text_affine_rgba_load_kernel(TextAffineArgs a) { affine_colour_rows<N, FILL, BLEND, false, true>(a); }
template <int N, int FILL, int BLEND>
FR_TEXT_GLOBAL text_affine_srgb_load_kernel(TextAffineArgs a) { affine_colour_rows<N, FILL, BLEND, true, true>(a); }
#undef FR_TEXT_GLOBAL

namespace {

template <class ARGS, int FAM, int FILL, int BLEND, int N>
constexpr auto text_kernel_of() -> void (*)(ARGS)
{
    if constexpr (FAM == 0) return text_affine_kernel<N, FILL>;
    else if constexpr (FAM == 1) return text_affine_rgba_kernel<N, FILL, BLEND>;
    else if constexpr (FAM == 2) return text_affine_srgb_kernel<N, FILL, BLEND>;
    else if constexpr (FAM == 3) return text_affine_rgba_load_kernel<N, FILL, BLEND>;
    else return text_affine_srgb_load_kernel<N, FILL, BLEND>;
}

}  // namespace

hipError_t launch_text(const TextLaunch &e, const TextAffineArgs &a, hipStream_t stream)
{
    return launch_text_instance(e, a, stream, [](auto FAM, auto FILL, auto BLEND, auto N) { return text_kernel_of<TextAffineArgs, FAM, FILL, BLEND, N>(); });
}

}  // namespace fr

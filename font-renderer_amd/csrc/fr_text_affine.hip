// fr_text_affine.hip — text runs of fr_glyph_place_affine placements (include/fr_raster.h, DESIGN.md sections 4.7 and 5):
// every placement carries a 2 x 2 matrix, so text runs rotated, mirrored or along any direction.  The tile walk, the
// colour arithmetic, LOAD, sRGB and the stores are the two row bodies of fr_text.hip, unchanged; only the evaluation of an
// instance's mask differs (fr_text_affine_mask_kernel.inc): a sample row's ray height is no longer the same in all 64
// lanes, so every lane solves every record at its own height, and a wave-uniform cull skips the records whose height
// range the row's samples cannot reach.  A translation unit of its own: the 54 instances compile beside the 108 of
// fr_text.hip, and nothing here can move a register of those.
#include "fr_text.hpp"
#include "fr_srgb.hpp"
#include "fr_wave.hpp"

#include <cstdio>
#include <type_traits>

namespace fr {

// the colour arithmetic of fr_text_colour_kernel.inc (described in fr_text.hip)
__device__ __forceinline__ uint32_t blend2(uint32_t c2, uint32_t cA2, uint32_t ia)
{
    const uint32_t t = c2 * ia + cA2;
    return ((t + ((t >> 8) & 0x00ff00ffu)) >> 8) & 0x00ff00ffu;
}
__device__ __forceinline__ uint32_t srgb_encode(const uint16_t *K, uint32_t L)
{
    const uint32_t k = K[L >> 4];
    return (k & 0xffu) + ((L & 15u) >= (k >> 8) ? 1u : 0u);
}
__device__ __forceinline__ uint32_t div255_24(uint32_t y)
{
    return (uint32_t)(((uint64_t)(y & 0xffffffu) * 0x808081u) >> 31);
}
#ifndef FR_TEXT_LOAD_SKIP
#define FR_TEXT_LOAD_SKIP 1
#endif

// T, as a type that depends on N: the bodies name members of the other placement forms' instances in branches that
// if constexpr discards, which only a dependent type leaves unchecked (as in fr_text.hip)
template <int N, class T>
using dependent_t = std::conditional_t<(N > 0), T, void>;

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

template <class ARGS>
constexpr const char *text_form() { return "affine_"; }

template <class ARGS, int FAM, int FILL, int BLEND, int N>
constexpr auto text_kernel_of() -> void (*)(ARGS)
{
    if constexpr (FAM == 0) return text_affine_kernel<N, FILL>;
    else if constexpr (FAM == 1) return text_affine_rgba_kernel<N, FILL, BLEND>;
    else if constexpr (FAM == 2) return text_affine_srgb_kernel<N, FILL, BLEND>;
    else if constexpr (FAM == 3) return text_affine_rgba_load_kernel<N, FILL, BLEND>;
    else return text_affine_srgb_load_kernel<N, FILL, BLEND>;
}

#include "fr_text_launch.inc"

}  // namespace

template <>
hipError_t launch_text(const TextAffineArgs &a, int n, int fill, int rgba, int blend, int srgb, int load, uint32_t n_tiles,
                       hipStream_t stream, char *name, size_t name_cap)
{
    return launch_any(a, n, fill, rgba, blend, srgb, load, Launch{n_tiles, stream, name, name_cap});
}

}  // namespace fr

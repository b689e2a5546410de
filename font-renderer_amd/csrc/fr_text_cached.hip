// fr_text_cached.hip — FR_TEXT_CACHE text plans (include/fr_raster.h, DESIGN.md sections 4.7 and 5): each distinct (glyph,
// pen fraction, scale, slant) key of a plan is rasterised once per render into a mask cell, and every instance of the key
// reads its masks from that cell.  An instance's n^2-bit mask at a pixel depends only on the key and on the pixel's offset
// from the pen's whole-pixel part, so the bytes are those of the plan without the flag.
//
// glyph_mask_kernel: one workgroup of four waves per 64 x 16 tile of a mask cell, a wave on every fourth row, one cell
// column per lane.  The cell is an instance in the TextInstEx layout whose image is the whole cell (fr_text_tables.hpp), and
// the mask is the text of fr_text_mask_kernel.inc with PLACE = true, exactly as the cover body includes it; with fy = 0 and
// slant 0 that arithmetic is the upright form's bit for bit (include/fr_raster.h), so the six instances N x FILL serve both
// placement forms.  Every element of the cell is stored: 0 where the winding is zero.
//
// glyph_mask_affine_kernel: the same shape for FR_TEXT_CACHE_AFFINE plans (key: glyph, both pen fractions, the bits of the
// matrix); the cell is an instance in the TextInstAffine layout and the mask is the text of fr_text_affine_mask_kernel.inc.
// Six more instances N x FILL; the composites below serve these plans as they are.
//
// text_cached_*_kernel: the two row bodies of fr_text.hip — tile walk, row loop, instance loops, colour arithmetic, LOAD,
// sRGB, stores — compiled here with FR_TEXT_MASK_CACHED, which replaces the evaluation of an instance's mask by one 2-byte
// load from its key's cell, issued by the lanes inside the clipped cell only.  A preprocessor switch and a translation
// unit of its own: the instances of fr_text.hip and fr_text_affine.hip (162 when the cache went in) compile from the text they had.  The fill
// rule acts only where masks are made, and one record (TextCachedInst) serves both placement forms, so these instances
// carry neither FILL nor a form.
#include "fr_text.hpp"
#include "fr_text_colour.hpp"
#include "fr_srgb.hpp"
#include "fr_wave.hpp"

#include <type_traits>

namespace fr {

#define FR_TEXT_GLOBAL __global__ __launch_bounds__(64 * TEXT_WAVES) void
template <int N, int FILL>
FR_TEXT_GLOBAL glyph_mask_kernel(TextMaskArgs a)
{
    constexpr bool PLACE = true;
    const TextMaskTile tl = a.tiles[blockIdx.x];
    const TextMaskCell *cl = static_cast<const TextMaskCell *>(a.cells) + tl.cell;
    const dependent_t<N, TextInstEx> in = cl->in;
    [[maybe_unused]] const dependent_t<N, TextRun> rn{};                   // (named by the other form's branch of the mask text)
    uint16_t *cell = a.masks + cl->base;
    const int lane = (int)(threadIdx.x & 63u);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int X = (int)tl.x0 + lane;
    float off[N];
#pragma unroll
    for (int k = 0; k < N; ++k) off[k] = sub_off(k, N, a.phase_center);
    for (int yy = wave; yy < TEXT_TILE_H; yy += TEXT_WAVES) {
        const int Y = (int)tl.y0 + yy;
        if (Y >= in.y1) break;                                             // (x1 = cw, y1 = ch: the whole cell)
        uint32_t m;
#include "fr_text_mask_kernel.inc"
        if (X < in.x1) cell[(uint32_t)Y * (uint32_t)in.x1 + (uint32_t)X] = (uint16_t)m;
    }
}

// The same for the cells of an FR_TEXT_CACHE_AFFINE plan (TextMaskCellAffine): the mask is the text of
// fr_text_affine_mask_kernel.inc, exactly as the row bodies of fr_text_affine.hip include it, with `inside` the lanes left of
// cw.  The map reads X and Y only through f32(X - ix) and f32(iy - Y), which in the cell are the small integers they are in
// a run (ix = -min_x, iy = max_y), so the bits are those of every instance of the key.  Lanes right of cw stay out of the
// cull range [cmin, cmax] and store nothing; a wave row is inside the cell in its first lane or not at all (Y < ch and
// tl.x0 < cw), so no row runs the record loop for nobody.
template <int N, int FILL>
FR_TEXT_GLOBAL glyph_mask_affine_kernel(TextMaskArgs a)
{
    const TextMaskTile tl = a.tiles[blockIdx.x];
    const TextMaskCellAffine *cl = static_cast<const TextMaskCellAffine *>(a.cells) + tl.cell;
    const dependent_t<N, TextInstAffine> in = cl->in;
    uint16_t *cell = a.masks + cl->base;
    const int lane = (int)(threadIdx.x & 63u);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int X = (int)tl.x0 + lane;
    float off[N];
#pragma unroll
    for (int k = 0; k < N; ++k) off[k] = sub_off(k, N, a.phase_center);
    for (int yy = wave; yy < TEXT_TILE_H; yy += TEXT_WAVES) {
        const int Y = (int)tl.y0 + yy;
        if (Y >= in.y1) break;                                             // (x1 = cw, y1 = ch: the whole cell)
        const bool inside = X < in.x1;
        uint32_t m;
#include "fr_text_affine_mask_kernel.inc"
        if (inside) cell[(uint32_t)Y * (uint32_t)in.x1 + (uint32_t)X] = (uint16_t)m;
    }
}

#define FR_TEXT_MASK_CACHED 1
template <int N>
FR_TEXT_GLOBAL text_cached_kernel(TextCachedArgs a)
{
    using INST = TextCachedInst;
#include "fr_text_cover_kernel.inc"
}
template <int N, int BLEND, bool SRGB, bool LOAD>
__device__ __forceinline__ void cached_colour_rows(const TextCachedArgs &a)
{
    using INST = TextCachedInst;
#include "fr_text_colour_kernel.inc"
}
template <int N, int BLEND>
FR_TEXT_GLOBAL text_cached_rgba_kernel(TextCachedArgs a) { cached_colour_rows<N, BLEND, false, false>(a); }
template <int N, int BLEND>
FR_TEXT_GLOBAL text_cached_srgb_kernel(TextCachedArgs a) { cached_colour_rows<N, BLEND, true, false>(a); }
template <int N, int BLEND>
FR_TEXT_GLOBAL text_cached_rgba_load_kernel(TextCachedArgs a) { cached_colour_rows<N, BLEND, false, true>(a); }
template <int N, int BLEND>
FR_TEXT_GLOBAL text_cached_srgb_load_kernel(TextCachedArgs a) { cached_colour_rows<N, BLEND, true, true>(a); }
#undef FR_TEXT_MASK_CACHED
#undef FR_TEXT_GLOBAL

namespace {

// FAM (TextLaunch::colour): 0 coverage (no BLEND), 1 rgba, 2 srgb, 3 rgba load, 4 srgb load
template <int FAM, int BLEND, int N>
constexpr auto cached_kernel_of() -> void (*)(TextCachedArgs)
{
    if constexpr (FAM == 0) return text_cached_kernel<N>;
    else if constexpr (FAM == 1) return text_cached_rgba_kernel<N, BLEND>;
    else if constexpr (FAM == 2) return text_cached_srgb_kernel<N, BLEND>;
    else if constexpr (FAM == 3) return text_cached_rgba_load_kernel<N, BLEND>;
    else return text_cached_srgb_load_kernel<N, BLEND>;
}

}  // namespace

hipError_t launch_glyph_mask(const TextLaunch &e, const TextMaskArgs &a, hipStream_t stream)
{
    const int key[] = {e.form, e.n, e.fill};
    return pick(key, [&](auto FORM, auto N, auto FILL) {
        if constexpr (decltype(FORM)::value == TEXT_AFFINE) return launch_tiles<TextMaskArgs>(glyph_mask_affine_kernel<N, FILL>, e.grid, stream, a);
        else return launch_tiles<TextMaskArgs>(glyph_mask_kernel<N, FILL>, e.grid, stream, a);
    }, Among<TEXT_PLAIN, TEXT_EX, TEXT_AFFINE>{}, Among<1, 2, 4>{}, Among<0, 1>{});
}

hipError_t launch_text_cached(const TextLaunch &e, const TextCachedArgs &a, hipStream_t stream)
{
    const int key[] = {e.colour, e.blend, e.n};
    return pick(key, [&](auto FAM, auto BLEND, auto N) {
        if constexpr (decltype(FAM)::value == 0 && decltype(BLEND)::value != 0) return hipErrorInvalidValue;
        else return launch_tiles(cached_kernel_of<FAM, BLEND, N>(), e.grid, stream, a);
    }, Among<0, 1, 2, 3, 4>{}, Among<0, 1, 2>{}, Among<1, 2, 4>{});
}

}  // namespace fr

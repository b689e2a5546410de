// fr_host_rules.hpp — the host arithmetic of the C ABI that needs no device (fr_host_rules.cpp): plain C++ compiled with
// -ffp-contract=off, so its binary32 steps round one by one as render_glyph.zig's do.  Besides what it declares here the
// unit holds the entry points fr_render_glyph_dims, fr_atlas_layout, fr_atlas_layout_glyph_dims, fr_srgb_decode,
// fr_srgb_encode and fr_rgba_unpremultiply.  Errors go through fr::set_error.  host/host_rules_selftest.cpp runs all of it
// on the CPU.
#pragma once
#include "../../include/fr_raster.h"

#include <cstddef>

namespace fr {

int check_params(const fr_raster_params *p);
// the bits an entry point takes besides FR_FILL_CONSISTENT (the RGBA text entry points: FR_TEXT_SRGB, FR_TEXT_BGRA,
// FR_TEXT_LOAD, FR_TEXT_OVER; the four upright and _ex text entry points: FR_TEXT_CACHE; the two _affine ones:
// FR_TEXT_CACHE_AFFINE)
int check_flags(uint32_t flags, uint32_t also = 0u);
// what job j must satisfy for the kernels' arithmetic to be the reference's (a plan's jobs, and the cells
// fr_selftest_row_cuts walks), against a glyph set of n_glyphs
int check_job(uint32_t n_glyphs, const fr_job &jb, uint32_t j);
// the lattice of the exact-integer path: 128-bit predicates hold dy*abxy^2 < 2^106 * K^6 for i16 points scaled by K
int check_k(uint32_t K, int32_t x0, int32_t y0, uint64_t w, uint64_t h);
// the scale of a job (check_job, fr_render_glyph): keeps every ray height, quotient and FMA residual of div_by_int inside
// the normal range (the reference's own scale = u16 / u16 lies in [2^-16, 2^16])
inline bool scale_in_range(float s) { return !(s < 9.5367431640625e-07f || s > 1048576.0f); }

// The device arena of fr_render_glyph for a glyph of np points and ns segments and an image of img_bytes, as byte offsets
// (every part 16-byte aligned).  [0, up) is uploaded in one copy: points, first-point indices, per-segment points, the
// glyph's segment range, the job, its segment range and the list of large glyphs; behind it the record counts, the
// records (rec_bytes each, two per segment) and the image.
struct GlyphArena {
    size_t pts, p0, spts, gseg, job, jseg, large, up, cnt, recs, out, total;
};
GlyphArena glyph_arena(uint64_t np, uint32_t ns, size_t rec_bytes, size_t img_bytes);

}  // namespace fr

// fr_host_rules.cpp — the host arithmetic of the C ABI that needs no device (fr_host_rules.hpp): the argument checks, the
// image size of renderGlyph, both atlas layouts, the sRGB conversions, and fr_render_glyph's arena layout.  No HIP.
#include "fr_host_rules.hpp"
#include "fr_srgb.hpp"

#include <algorithm>
#include <cmath>

namespace fr {

int set_error(int code, const char *fmt, ...);         // the context unit (the self-test has its own)

int check_params(const fr_raster_params *p)
{
    if (!p) return set_error(FR_E_INVALID, "params is NULL");
    if (p->mode < FR_WINDING_I16 || p->mode > FR_SDF_U8) return set_error(FR_E_INVALID, "unknown mode %d", p->mode);
    const int n = p->samples_per_axis;
    if (p->mode == FR_COVERAGE_U8) {
        if (n != 1 && n != 2 && n != 4) return set_error(FR_E_UNSUPPORTED, "samples_per_axis %d not in {1,2,4}", n);
    } else if (n != 1) {
        return set_error(FR_E_INVALID, "samples_per_axis must be 1 for mode %d", p->mode);
    }
    if (p->sample_phase != FR_SAMPLE_CORNER && p->sample_phase != FR_SAMPLE_CENTER)
        return set_error(FR_E_INVALID, "unknown sample_phase %d", p->sample_phase);
    return FR_OK;
}

int check_flags(uint32_t flags, uint32_t also)
{
    const uint32_t known = (uint32_t)FR_FILL_CONSISTENT | also;
    if (flags & ~known) return set_error(FR_E_INVALID, "unknown flag bits 0x%x", flags & ~known);
    return FR_OK;
}

int check_job(uint32_t n_glyphs, const fr_job &jb, uint32_t j)
{
    if (jb.glyph >= n_glyphs) return set_error(FR_E_INVALID, "job %u: glyph %u of %u", j, jb.glyph, n_glyphs);
    if (!(jb.scale > 0.0f) || !std::isfinite(jb.scale)) return set_error(FR_E_INVALID, "job %u: scale must be finite and > 0", j);
    if (!scale_in_range(jb.scale)) return set_error(FR_E_UNSUPPORTED, "job %u: scale outside [2^-20, 2^20]", j);
    if (jb.w > 65535u || jb.h > 65535u) return set_error(FR_E_UNSUPPORTED, "job %u: cell larger than 65535", j);
    // sample coordinates must be exactly representable in binary32
    if (jb.min_x < -(1 << 22) || (int64_t)jb.min_x + jb.w > (1 << 22) || jb.max_y > (1 << 22) ||
        (int64_t)jb.max_y - jb.h < -(1 << 22))
        return set_error(FR_E_UNSUPPORTED, "job %u: pixel coordinates beyond +-2^22", j);
    return FR_OK;
}

// K <= 8 cannot overflow
int check_k(uint32_t K, int32_t x0, int32_t y0, uint64_t w, uint64_t h)
{
    if (K < 1 || K > 8) return set_error(FR_E_UNSUPPORTED, "K must be in [1, 8] (128-bit predicate range)");
    if (w > (1u << 20) || h > (1u << 20)) return set_error(FR_E_UNSUPPORTED, "lattice larger than 2^20 per axis");
    const int64_t lim = (int64_t)1 << 20;           // query points stay within a few em of the scaled glyph
    if (x0 < -lim || x0 + (int64_t)w > lim || y0 > lim || y0 - (int64_t)h < -lim)
        return set_error(FR_E_UNSUPPORTED, "lattice beyond +-2^20 scaled units");
    return FR_OK;
}

GlyphArena glyph_arena(uint64_t np, uint32_t ns, size_t rec_bytes, size_t img_bytes)
{
    auto al = [](size_t v) { return (v + 15u) & ~(size_t)15; };
    GlyphArena a;
    a.pts = 0;
    a.p0 = al(a.pts + np * 4 + 16);
    a.spts = al(a.p0 + (size_t)ns * 4 + 4);
    a.gseg = al(a.spts + (size_t)ns * 12 + 16);
    a.job = al(a.gseg + 8);
    a.jseg = al(a.job + sizeof(fr_job));
    a.large = al(a.jseg + 8);
    a.up = al(a.large + 4);
    a.cnt = a.up;
    a.recs = al(a.cnt + 8);
    a.out = al(a.recs + (size_t)(ns ? ns : 1) * 2 * rec_bytes);
    a.total = al(a.out + img_bytes);
    return a;
}

}  // namespace fr

using fr::set_error;

extern "C" {

// ---- renderGlyph drop-in ----------------------------------------------------
// render_glyph.zig:13-19, host arithmetic in binary32 exactly as written there.
int fr_render_glyph_dims(const int16_t box[4], uint16_t units_per_em, uint16_t font_size,
                         int16_t min_corner[2], int16_t max_corner[2], uint16_t *width,
                         uint16_t *height, float *scale_out)
{
    if (!box || !min_corner || !max_corner || !width || !height) return set_error(FR_E_INVALID, "fr_render_glyph_dims: NULL argument");
    if (units_per_em == 0 || font_size == 0) return set_error(FR_E_INVALID, "units_per_em and font_size must be > 0");
    const float scale = (float)font_size / (float)units_per_em;                    // :13
    const float b[4] = {(float)box[0] * scale, (float)box[1] * scale, (float)box[2] * scale, (float)box[3] * scale};   // :15
    const float lo0 = std::floor(b[0]), lo1 = std::floor(b[1]), hi0 = std::ceil(b[2]), hi1 = std::ceil(b[3]);
    if (lo0 < -32768.f || lo1 < -32768.f || hi0 > 32767.f || hi1 > 32767.f)
        return set_error(FR_E_UNSUPPORTED, "scaled box leaves i16 (the reference's @intFromFloat would trap)");
    min_corner[0] = (int16_t)lo0; min_corner[1] = (int16_t)lo1;                    // :16
    max_corner[0] = (int16_t)hi0; max_corner[1] = (int16_t)hi1;                    // :17
    const int w = (int)max_corner[0] - min_corner[0] + 1, h = (int)max_corner[1] - min_corner[1] + 1;   // :18-19
    if (w < 1 || h < 1 || w > 32767 || h > 32767) return set_error(FR_E_UNSUPPORTED, "image size leaves i16");
    *width = (uint16_t)w; *height = (uint16_t)h;
    if (scale_out) *scale_out = scale;
    return FR_OK;
}

int fr_atlas_layout(const int16_t *boxes, uint32_t n_glyphs, uint32_t first_glyph,
                    const uint16_t *units_per_em, uint32_t n_upm, uint16_t font_size,
                    uint32_t cell, uint32_t cols, uint32_t rows_per_page,
                    fr_job *jobs_out, uint32_t *page_of_job, uint32_t *n_pages)
{
    if (n_glyphs && (!boxes || !jobs_out)) return set_error(FR_E_INVALID, "fr_atlas_layout: NULL argument");
    if (!units_per_em || (n_upm != 1 && n_upm != n_glyphs)) return set_error(FR_E_INVALID, "units_per_em: one value or one per glyph");
    if (cell == 0 || cols == 0 || font_size == 0) return set_error(FR_E_INVALID, "cell, cols and font_size must be > 0");
    if ((uint64_t)cell * cols > 0xffffffffull) return set_error(FR_E_UNSUPPORTED, "atlas wider than 2^32 pixels");
    const uint64_t per_page = rows_per_page ? (uint64_t)rows_per_page * cols : 0;
    for (uint32_t i = 0; i < n_glyphs; ++i) {
        const uint16_t upm = units_per_em[n_upm == 1 ? 0 : i];
        if (upm == 0) return set_error(FR_E_INVALID, "units_per_em must be > 0");
        const float scale = (float)font_size / (float)upm;                              // render_glyph.zig:13
        const float fx = std::floor((float)boxes[4 * (size_t)i + 0] * scale);           // :15-16
        const float fy = std::ceil((float)boxes[4 * (size_t)i + 3] * scale);            // :15, :17
        const uint64_t slot = per_page ? i % per_page : i;
        const uint64_t row = slot / cols;
        if (row * cell > 0xffffffffull) return set_error(FR_E_UNSUPPORTED, "atlas taller than 2^32 pixels: use pages");
        fr_job &jb = jobs_out[i];
        jb.glyph = first_glyph + i;
        jb.min_x = (int32_t)fx; jb.max_y = (int32_t)fy;
        jb.w = cell; jb.h = cell;
        jb.out_x = (uint32_t)(slot % cols) * cell;
        jb.out_y = (uint32_t)row * cell;
        jb.scale = scale;
        if (page_of_job) page_of_job[i] = per_page ? (uint32_t)(i / per_page) : 0u;
    }
    if (n_pages) *n_pages = per_page ? (uint32_t)((n_glyphs + per_page - 1) / per_page) : (n_glyphs ? 1u : 0u);
    return FR_OK;
}

// renderGlyph's own image per glyph (render_glyph.zig:13-19 through fr_render_glyph_dims), shelf-packed in input order
int fr_atlas_layout_glyph_dims(const int16_t *boxes, uint32_t n_glyphs, uint32_t first_glyph,
                               const uint16_t *units_per_em, uint32_t n_upm, uint16_t font_size,
                               uint32_t atlas_w, uint32_t align, fr_job *jobs_out, uint32_t *atlas_h)
{
    if (n_glyphs && (!boxes || !jobs_out)) return set_error(FR_E_INVALID, "fr_atlas_layout_glyph_dims: NULL argument");
    if (!units_per_em || (n_upm != 1 && n_upm != n_glyphs)) return set_error(FR_E_INVALID, "units_per_em: one value or one per glyph");
    if (atlas_w == 0 || font_size == 0) return set_error(FR_E_INVALID, "atlas_w and font_size must be > 0");
    if (align == 0) align = 1;
    uint64_t x = 0, y = 0, shelf_h = 0;
    for (uint32_t i = 0; i < n_glyphs; ++i) {
        int16_t mn[2], mx[2];
        uint16_t w, h;
        float scale;
        const int rc = fr_render_glyph_dims(boxes + 4 * (size_t)i, units_per_em[n_upm == 1 ? 0 : i], font_size, mn, mx, &w, &h, &scale);
        if (rc) return rc;
        if (w > atlas_w) return set_error(FR_E_INVALID, "glyph %u is %u pixels wide, the atlas %u", i, (unsigned)w, atlas_w);
        x = (x + align - 1) / align * align;
        if (x + w > atlas_w) { x = 0; y += shelf_h; shelf_h = 0; }          // next shelf
        if (y + h > 0xffffffffull) return set_error(FR_E_UNSUPPORTED, "atlas taller than 2^32 pixels");
        fr_job &jb = jobs_out[i];
        jb.glyph = first_glyph + i;
        jb.min_x = mn[0]; jb.max_y = mx[1];                                  // :26-27: sample (min_x + x, max_y - y)
        jb.w = w; jb.h = h;
        jb.out_x = (uint32_t)x; jb.out_y = (uint32_t)y;
        jb.scale = scale;
        x += w;
        shelf_h = std::max<uint64_t>(shelf_h, h);
    }
    if (atlas_h) *atlas_h = (uint32_t)std::min<uint64_t>(y + shelf_h, 0xffffffffull);
    return FR_OK;
}

// the conversions of FR_TEXT_SRGB plans, from the tables text_srgb_kernel reads (fr_srgb.hpp)
int fr_srgb_decode(const uint8_t *in, size_t n, uint16_t *out)
{
    if (n && (!in || !out)) return set_error(FR_E_INVALID, "fr_srgb_decode: NULL argument");
    for (size_t i = 0; i < n; ++i) out[i] = fr::SRGB_D[in[i]];
    return FR_OK;
}

int fr_srgb_encode(const uint16_t *in, size_t n, uint8_t *out)
{
    if (n && (!in || !out)) return set_error(FR_E_INVALID, "fr_srgb_encode: NULL argument");
    for (size_t i = 0; i < n; ++i) {
        const uint32_t L = in[i], k = fr::SRGB_K[L >> 4];
        out[i] = (uint8_t)((k & 0xffu) + ((L & 15u) >= (k >> 8) ? 1u : 0u));
    }
    return FR_OK;
}

// premultiplied -> straight alpha, in place (the output of FR_TEXT_OVER plans; include/fr_raster.h)
int fr_rgba_unpremultiply(uint8_t *rgba, size_t n_pixels, int srgb)
{
    if (n_pixels && !rgba) return set_error(FR_E_INVALID, "fr_rgba_unpremultiply: NULL argument");
    for (size_t i = 0; i < n_pixels; ++i) {
        uint8_t *p = rgba + 4 * i;
        const uint32_t a = p[3];
        if (a == 0u) { p[0] = p[1] = p[2] = 0; continue; }
        for (int c = 0; c < 3; ++c) {
            if (srgb) {
                const uint32_t L = std::min<uint32_t>(65535u, (255u * fr::SRGB_D[p[c]] + a / 2u) / a), k = fr::SRGB_K[L >> 4];
                p[c] = (uint8_t)((k & 0xffu) + ((L & 15u) >= (k >> 8) ? 1u : 0u));
            } else {
                p[c] = (uint8_t)std::min<uint32_t>(255u, (255u * p[c] + a / 2u) / a);
            }
        }
    }
    return FR_OK;
}

}  // extern "C"

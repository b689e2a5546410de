// fr_host.hpp — C++ host-side mirror of the reference's interface for this path, sitting on
// the C ABI (include/fr_raster.h).  The reference is compiled code (Zig) and no Zig toolchain
// exists in the build image, so this header is the compiled-language host a maintainer can
// read next to the Zig: same names, argument meaning and error behaviour as
//   /root/reference/src/font/Glyph.zig:11-24          (Glyph, Box, Contour)
//   /root/reference/src/font/Font.zig:25-29           (Font::Information)
//   /root/reference/src/tools/Image.zig:44-130        (Image::Gray, Image::Winding)
//   /root/reference/src/tools/render_glyph.zig:11,160 (renderGlyph, windingInGlyph)
// Nothing is computed here: every call goes to libfr_raster.so (HIP, gfx950).
#pragma once
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/fr_raster.h"

namespace fr_host {

struct Point { int16_t x, y; };                       // geometry.zig:7-11 (extern struct)
struct Box { int16_t x_min = 0, y_min = 0, x_max = 0, y_max = 0; };   // Glyph.zig:15-20
struct Contour { std::vector<Point> points; };        // Glyph.zig:22-24: even on-curve, odd control, last == first
struct Glyph {                                        // Glyph.zig:11-12
    Box box;
    std::vector<Contour> contours;
    static Glyph initEmpty() { return {}; }           // Glyph.zig:77-82
};
struct FontInformation { uint16_t units_per_em; bool y0_baseline = true; };   // Font.zig:25-29

struct RasterFailed : std::runtime_error {            // the Zig shim's error.RasterFailed
    int code;
    RasterFailed(int c, const char *m) : std::runtime_error(m), code(c) {}
};
inline void check(int rc) { if (rc != FR_OK) throw RasterFailed(rc, fr_last_error()); }

namespace Image {
struct Gray {                                         // Image.zig:44-83
    uint32_t width = 0, height = 0;
    std::vector<uint8_t> data;                        // row-major, y*width + x
    static Gray init(uint32_t w, uint32_t h) { Gray g; g.width = w; g.height = h; g.data.assign((size_t)w * h, 0); return g; }
    void getRGBLinear(size_t index, uint8_t rgb[3]) const { rgb[0] = rgb[1] = rgb[2] = data[index]; }   // :78-82
};
struct Winding {                                      // Image.zig:85-130
    uint32_t width = 0, height = 0;
    std::vector<int16_t> data;
    uint8_t scaler = 50, overflow_color = 150;
    static Winding init(uint32_t w, uint32_t h, uint8_t scaler, uint8_t overflow) {
        Winding g; g.width = w; g.height = h; g.data.assign((size_t)w * h, 0); g.scaler = scaler; g.overflow_color = overflow; return g;
    }
    void getRGBLinear(size_t index, uint8_t rgb[3]) const {                                             // :121-129
        const int16_t val = data[index];
        if (val == 0) { rgb[0] = rgb[1] = rgb[2] = 0; return; }
        uint32_t c = (uint32_t)scaler * (uint32_t)(val < 0 ? -val : val);
        if (c > 65535u) c = 65535u;                   // u16 saturating multiply
        const uint8_t color = (uint8_t)(c > 255u ? 255u : c);
        const uint8_t sub = (c == color) ? 0 : overflow_color;
        if (val > 0) { rgb[0] = sub; rgb[1] = sub; rgb[2] = color; } else { rgb[0] = color; rgb[1] = sub; rgb[2] = sub; }
    }
};
struct RGB {                                          // Image.zig:132-170
    uint32_t width = 0, height = 0;
    std::vector<uint8_t> data;                        // row-major RGB triples
    static RGB init(uint32_t w, uint32_t h) { RGB g; g.width = w; g.height = h; g.data.assign((size_t)w * h * 3, 0); return g; }
    void getRGBLinear(size_t index, uint8_t rgb[3]) const { rgb[0] = data[3 * index]; rgb[1] = data[3 * index + 1]; rgb[2] = data[3 * index + 2]; }
};
struct GlyphDebug {                                   // Image.zig:173-241
    RGB rgb;
    uint8_t winding_scale = 50, overflow_color = 150;
};
}  // namespace Image

class Context {
public:
    explicit Context(int device = 0, void *stream = nullptr) { check(fr_ctx_create(device, stream, &h_)); }
    ~Context() { fr_ctx_destroy(h_); }
    Context(const Context &) = delete;
    Context &operator=(const Context &) = delete;
    fr_ctx *get() const { return h_; }
private:
    fr_ctx *h_ = nullptr;
};

// flat view the C ABI takes: points back to back + contour offsets
struct Flat {
    std::vector<int16_t> pts;
    std::vector<uint32_t> cstart{0};
    explicit Flat(const Glyph &g) {
        for (const Contour &c : g.contours) {
            for (const Point &p : c.points) { pts.push_back(p.x); pts.push_back(p.y); }
            cstart.push_back((uint32_t)(pts.size() / 2));
        }
        if (pts.empty()) pts.assign(2, 0);
    }
    uint32_t n_contours() const { return (uint32_t)cstart.size() - 1; }
};

// render_glyph.zig:11 — pub fn renderGlyph(glyph, font_info, font_size) !Image.Gray
inline Image::Gray renderGlyph(Context &ctx, const Glyph &glyph, FontInformation font_info, uint16_t font_size)
{
    const int16_t box[4] = {glyph.box.x_min, glyph.box.y_min, glyph.box.x_max, glyph.box.y_max};
    int16_t mn[2], mx[2];
    uint16_t w, h;
    check(fr_render_glyph_dims(box, font_info.units_per_em, font_size, mn, mx, &w, &h, nullptr));
    Image::Gray im = Image::Gray::init(w, h);                                   // :22
    Flat f(glyph);
    check(fr_render_glyph(ctx.get(), f.pts.data(), f.cstart.data(), f.n_contours(), box, font_info.units_per_em,
                          font_size, FR_GRAY_DEBUG, im.data.data()));
    return im;
}

// same grid, raw winding numbers (glyphWindingAt, :35-73) into an Image::Winding
inline Image::Winding renderGlyphWinding(Context &ctx, const Glyph &glyph, FontInformation font_info, uint16_t font_size)
{
    const int16_t box[4] = {glyph.box.x_min, glyph.box.y_min, glyph.box.x_max, glyph.box.y_max};
    int16_t mn[2], mx[2];
    uint16_t w, h;
    check(fr_render_glyph_dims(box, font_info.units_per_em, font_size, mn, mx, &w, &h, nullptr));
    Image::Winding im = Image::Winding::init(w, h, 50, 150);
    Flat f(glyph);
    check(fr_render_glyph(ctx.get(), f.pts.data(), f.cstart.data(), f.n_contours(), box, font_info.units_per_em,
                          font_size, FR_WINDING_I16, im.data.data()));
    return im;
}

// render_glyph.zig:160 — windingInGlyph(glyph, glyph_info, point) i16 (GlyphInfo is recomputed on the device)
inline int16_t windingInGlyph(Context &ctx, const Glyph &glyph, Point p)
{
    Flat f(glyph);
    const int16_t q[2] = {p.x, p.y};
    int16_t out = 0;
    check(fr_winding_in_glyph(ctx.get(), f.pts.data(), f.cstart.data(), f.n_contours(), q, 1, &out));
    return out;
}

// Image.zig:220 — Image.GlyphDebug.render(glyph, winding_scale): the exact-integer lattice coloured, points marked
inline Image::GlyphDebug glyphDebugRender(Context &ctx, const Glyph &glyph, uint8_t winding_scale)
{
    const int16_t box[4] = {glyph.box.x_min, glyph.box.y_min, glyph.box.x_max, glyph.box.y_max};
    Image::GlyphDebug im;
    im.winding_scale = winding_scale;
    im.rgb = Image::RGB::init((uint32_t)(box[2] - box[0] + 3), (uint32_t)(box[3] - box[1] + 3));     // :183
    Flat f(glyph);
    check(fr_glyph_debug_render(ctx.get(), f.pts.data(), f.cstart.data(), f.n_contours(), box, winding_scale, im.rgb.data.data()));
    return im;
}

// a batch of glyphs -> one atlas (build-defined cell grid, fr_atlas_layout) of n x n-sample coverage
// optional multi-GPU assembly (include/fr_raster.h): rank r rendered its band at atlas_dev + r * band_bytes; comm is the
// host's ncclComm_t
inline void allgatherBands(Context &ctx, void *nccl_comm, void *atlas_dev, size_t band_bytes)
{
    check(fr_allgather_bands(ctx.get(), nccl_comm, atlas_dev, band_bytes));
}

inline Image::Gray renderAtlas(Context &ctx, const std::vector<Glyph> &glyphs, FontInformation font_info, uint16_t font_size,
                               uint32_t cell, uint32_t cols, int samples_per_axis)
{
    std::vector<int16_t> pts, boxes;
    std::vector<uint32_t> cstart{0}, gstart{0};
    for (const Glyph &g : glyphs) {
        for (const Contour &c : g.contours) {
            for (const Point &p : c.points) { pts.push_back(p.x); pts.push_back(p.y); }
            cstart.push_back((uint32_t)(pts.size() / 2));
        }
        gstart.push_back((uint32_t)cstart.size() - 1);
        boxes.insert(boxes.end(), {g.box.x_min, g.box.y_min, g.box.x_max, g.box.y_max});
    }
    if (pts.empty()) pts.assign(2, 0);
    const uint32_t n = (uint32_t)glyphs.size();
    std::vector<fr_job> jobs(n ? n : 1);
    const uint16_t upm = font_info.units_per_em;
    check(fr_atlas_layout(boxes.data(), n, 0, &upm, 1, font_size, cell, cols, 0, jobs.data(), nullptr, nullptr));
    fr_glyphset *gs = nullptr;
    check(fr_glyphset_create(ctx.get(), pts.data(), cstart.data(), (uint32_t)cstart.size() - 1, gstart.data(), n, &gs));
    const uint32_t rows = (n + cols - 1) / cols;
    Image::Gray im = Image::Gray::init(cols * cell, rows * cell);
    fr_raster_params prm{FR_COVERAGE_U8, samples_per_axis, FR_SAMPLE_CENTER, 0};
    const int rc = fr_render_batch(ctx.get(), gs, jobs.data(), n, &prm, im.data.data(), (size_t)cols * cell, (size_t)rows * cell);
    fr_glyphset_destroy(gs);
    check(rc);
    return im;
}

// a text plan of fr_glyph_place_ex placements (include/fr_raster.h: own scale, slant and sub-pixel baseline per placement)
// or of fr_glyph_place_affine placements (a 2 x 2 matrix per placement: rotated, mirrored and sheared text; the struct is
// the C header's: uint32_t glyph, int32_t pen_x64, pen_y64, float m[4] = xx, xy, yx, yy) over a set of glyphs: coverage bytes, or RGBA pixels when place_rgba is given.  The plan renders into DEVICE memory
// (fr_plan_render), which the host that owns the HIP stream allocates; this mirror owns the glyph set and the plan.
// flags: the header's, passed through; with place_rgba FR_TEXT_OVER (256) makes the pixels premultiplied R G B A with
// source-over alpha, which unpremultiply() below turns into straight alpha once they are back on the host.
inline void unpremultiply(std::vector<uint8_t> &rgba, bool srgb = false) { check(fr_rgba_unpremultiply(rgba.data(), rgba.size() / 4, srgb ? 1 : 0)); }

// fr_layer_over: rectangles of a finished premultiplied layer (a FR_TEXT_OVER render over a (0, 0, 0, 0) clear colour) over
// a premultiplied image, both in DEVICE memory the host owns, 4 bytes per pixel with alpha last; strides and rows count
// pixels.  Asynchronous on the context's stream; `blits` may be reused at once.  srgb: FR_LAYER_SRGB (both images are
// premultiplied in linear light).  A viewer renders the layer once and calls this per frame with the frame's offset.
struct DeviceImage {
    void *pixels;
    size_t stride_px, rows;
};
inline void layer_over(Context &ctx, const DeviceImage &layer, const DeviceImage &image, const std::vector<fr_layer_blit> &blits, bool srgb = false)
{
    check(fr_layer_over(ctx.get(), layer.pixels, layer.stride_px, layer.rows, image.pixels, image.stride_px, image.rows, blits.data(),
                        (uint32_t)blits.size(), srgb ? FR_LAYER_SRGB : 0u));
}
// fr_layer_unpremultiply: unpremultiply() above on the device, over the w x h window at the image's first pixel
inline void layer_unpremultiply(Context &ctx, const DeviceImage &image, uint32_t w, uint32_t h, bool srgb = false)
{
    check(fr_layer_unpremultiply(ctx.get(), image.pixels, image.stride_px, w, h, srgb ? 1 : 0));
}
// fr_layer_shadow: the alpha of a window of the layer, spread, box-blurred, moved by whole pixels and tinted, written as a
// premultiplied R G B A layer over every pixel of the rectangle of `image` that `shadow` names.  Composite the result with
// layer_over, then the text over it.  Asynchronous on the context's stream; `shadow` may be reused at once.
inline void layer_shadow(Context &ctx, const DeviceImage &layer, const DeviceImage &image, const fr_layer_shadow_params &shadow, bool srgb = false)
{
    check(fr_layer_shadow(ctx.get(), layer.pixels, layer.stride_px, layer.rows, image.pixels, image.stride_px, image.rows, &shadow,
                          srgb ? FR_LAYER_SRGB : 0u));
}
// fr_layer_outline: the alpha of a window of the layer grown or shrunk by a disc of outline.radius / 16 pixels, combined with
// the layer as outline.kind says (FR_OUTLINE_GROW / _RING / _INNER / _SHRINK), moved by whole pixels and tinted, written as a
// premultiplied R G B A layer over every pixel of the rectangle of `image` that `outline` names.  Composite a GROW outline
// with layer_over, then the text over it; an INNER line goes over the text.  Asynchronous on the context's stream; `outline`
// may be reused at once.
inline void layer_outline(Context &ctx, const DeviceImage &layer, const DeviceImage &image, const fr_layer_outline_params &outline, bool srgb = false)
{
    check(fr_layer_outline(ctx.get(), layer.pixels, layer.stride_px, layer.rows, image.pixels, image.stride_px, image.rows, &outline,
                           srgb ? FR_LAYER_SRGB : 0u));
}
// fr_layer_rects: anti-aliased rectangles (edges in 1/64 pixel, one straight colour each) composited in order over the
// premultiplied `image`: underlines, strike-outs, highlights, carets, panels.  They may overlap.  Asynchronous on the
// context's stream; `rects` may be reused at once.
inline void layer_rects(Context &ctx, const DeviceImage &image, const std::vector<fr_layer_rect> &rects, bool srgb = false)
{
    check(fr_layer_rects(ctx.get(), image.pixels, image.stride_px, image.rows, rects.data(), (uint32_t)rects.size(), srgb ? FR_LAYER_SRGB : 0u));
}
// fr_layer_paint: the gradient of `paint` composited over the premultiplied `image` through the alpha of the window of
// `layer` that `paint` names: gradient text from a text layer, a gradient glow from a shadow.  Asynchronous on the
// context's stream; `paint` may be reused at once.
inline void layer_paint(Context &ctx, const DeviceImage &layer, const DeviceImage &image, const fr_layer_paint_params &paint, bool srgb = false)
{
    check(fr_layer_paint(ctx.get(), layer.pixels, layer.stride_px, layer.rows, image.pixels, image.stride_px, image.rows, &paint, srgb ? FR_LAYER_SRGB : 0u));
}
// the same through full coverage: a gradient panel of paint.w x paint.h (paint.src_x = paint.src_y = 0)
inline void layer_paint(Context &ctx, const DeviceImage &image, const fr_layer_paint_params &paint, bool srgb = false)
{
    check(fr_layer_paint(ctx.get(), nullptr, 0, 0, image.pixels, image.stride_px, image.rows, &paint, srgb ? FR_LAYER_SRGB : 0u));
}
// fr_layer_lcd: sub-pixel (LCD) text.  `plane` is a FR_COVERAGE_U8 render three times as wide as the text (a PlacedText
// of fr_glyph_place_affine rows with m = {3 s, 0, 0, s} and the pens' x tripled), one byte per element; each blit filters
// its window across sub-pixels (weights: FR_LCD_TAPS values that add up to 256, or nullptr for the default filter) and
// composites its colour over the premultiplied `image` with an alpha per colour byte.  bgr: the panel's stripes are B G R.
// Asynchronous on the context's stream; `blits` and `weights` may be reused at once.
struct DevicePlane {
    const void *bytes;
    size_t stride, rows;
};
inline void layer_lcd(Context &ctx, const DevicePlane &plane, const DeviceImage &image, const std::vector<fr_lcd_blit> &blits, const uint16_t *weights = nullptr,
                      bool srgb = false, bool bgr = false)
{
    check(fr_layer_lcd(ctx.get(), plane.bytes, plane.stride, plane.rows, image.pixels, image.stride_px, image.rows, blits.data(), (uint32_t)blits.size(), weights,
                       (srgb ? FR_LAYER_SRGB : 0u) | (bgr ? FR_LCD_BGR : 0u)));
}
// fr_layer_mask: layer_over with an opacity per pixel, t = m(k', o), where k is the alpha of the pixel of `mask` (a layer:
// a panel, a shadow, an outline) that a blit lays over the pixel and k' = 255 - k where the blit inverts: text clipped to a
// shape, pixels showing through text, a soft wipe.  Asynchronous on the context's stream; `blits` may be reused at once.
inline void layer_mask(Context &ctx, const DeviceImage &layer, const DeviceImage &mask, const DeviceImage &image, const std::vector<fr_layer_mask_blit> &blits,
                       bool srgb = false)
{
    check(fr_layer_mask(ctx.get(), layer.pixels, layer.stride_px, layer.rows, mask.pixels, mask.stride_px, mask.rows, image.pixels, image.stride_px, image.rows,
                        blits.data(), (uint32_t)blits.size(), srgb ? FR_LAYER_SRGB : 0u));
}
// the same through a plane of bytes (a FR_COVERAGE_U8 render; any alignment)
inline void layer_mask(Context &ctx, const DeviceImage &layer, const DevicePlane &mask, const DeviceImage &image, const std::vector<fr_layer_mask_blit> &blits,
                       bool srgb = false)
{
    check(fr_layer_mask(ctx.get(), layer.pixels, layer.stride_px, layer.rows, mask.bytes, mask.stride, mask.rows, image.pixels, image.stride_px, image.rows,
                        blits.data(), (uint32_t)blits.size(), (srgb ? FR_LAYER_SRGB : 0u) | FR_MASK_PLANE));
}
// FR_MASK_ERASE: no layer; the image is multiplied by 255 - t (destination-out): a knock-out, or underlines that skip the ink
// of a grown text layer.  A blit's src_x and src_y are not used.
inline void layer_erase(Context &ctx, const DeviceImage &mask, const DeviceImage &image, const std::vector<fr_layer_mask_blit> &blits, bool srgb = false)
{
    check(fr_layer_mask(ctx.get(), nullptr, 0, 0, mask.pixels, mask.stride_px, mask.rows, image.pixels, image.stride_px, image.rows, blits.data(),
                        (uint32_t)blits.size(), (srgb ? FR_LAYER_SRGB : 0u) | FR_MASK_ERASE));
}
inline void layer_erase(Context &ctx, const DevicePlane &mask, const DeviceImage &image, const std::vector<fr_layer_mask_blit> &blits, bool srgb = false)
{
    check(fr_layer_mask(ctx.get(), nullptr, 0, 0, mask.bytes, mask.stride, mask.rows, image.pixels, image.stride_px, image.rows, blits.data(),
                        (uint32_t)blits.size(), (srgb ? FR_LAYER_SRGB : 0u) | FR_MASK_PLANE | FR_MASK_ERASE));
}
// fr_layer_warp: windows of `layer` composited over `image` through an affine map each: a blit names the window, the
// rectangle of the image it owns and the inverse map in 1/65536 window pixel (u0, v0 at the centre of rectangle pixel
// (0, 0); ux, vx per column; uy, vy per row), sampled bilinearly in exact integers.  A viewer that zooms, spins or
// smooth-scrolls finished text calls this per frame.  Asynchronous on the context's stream; `blits` may be reused at once.
inline void layer_warp(Context &ctx, const DeviceImage &layer, const DeviceImage &image, const std::vector<fr_layer_warp_blit> &blits, bool srgb = false)
{
    check(fr_layer_warp(ctx.get(), layer.pixels, layer.stride_px, layer.rows, image.pixels, image.stride_px, image.rows, blits.data(), (uint32_t)blits.size(),
                        srgb ? FR_LAYER_SRGB : 0u));
}
// fr_layer_blend: layer_over with a blend mode in the place of source-over (mode: FR_BLEND_MULTIPLY, _SCREEN, _OVERLAY,
// _DARKEN, _LIGHTEN, _HARD_LIGHT, _DIFFERENCE, _EXCLUSION or _PLUS): a highlighter stroke multiplied over text, a glow
// screened or added, text differenced into a photo.  One mode per call.  Asynchronous on the context's stream; `blits`
// may be reused at once.
inline void layer_blend(Context &ctx, const DeviceImage &layer, const DeviceImage &image, const std::vector<fr_layer_blit> &blits, uint32_t mode, bool srgb = false)
{
    check(fr_layer_blend(ctx.get(), layer.pixels, layer.stride_px, layer.rows, image.pixels, image.stride_px, image.rows, blits.data(), (uint32_t)blits.size(),
                         mode, srgb ? FR_LAYER_SRGB : 0u));
}

class PlacedText {
public:
    PlacedText(Context &ctx, const std::vector<Glyph> &glyphs, const std::vector<fr_glyph_place_ex> &places,
               const std::vector<fr_text_run> &runs, int samples_per_axis = 4, uint32_t flags = 0,
               const std::vector<uint8_t> *place_rgba = nullptr, const std::vector<uint8_t> *run_clear_rgba = nullptr)
    {
        init(ctx, glyphs, places, runs, samples_per_axis, flags, place_rgba, run_clear_rgba);
    }
    PlacedText(Context &ctx, const std::vector<Glyph> &glyphs, const std::vector<fr_glyph_place_affine> &places,
               const std::vector<fr_text_run> &runs, int samples_per_axis = 4, uint32_t flags = 0,
               const std::vector<uint8_t> *place_rgba = nullptr, const std::vector<uint8_t> *run_clear_rgba = nullptr)
    {
        init(ctx, glyphs, places, runs, samples_per_axis, flags, place_rgba, run_clear_rgba);
    }
    ~PlacedText() { fr_plan_destroy(plan_); fr_glyphset_destroy(gs_); }
    PlacedText(const PlacedText &) = delete;
    PlacedText &operator=(const PlacedText &) = delete;
    fr_plan *get() const { return plan_; }
    uint64_t pixels() const { return fr_plan_pixels(plan_); }
    std::string describe() const
    {
        char buf[512];
        check(fr_plan_describe(plan_, buf, sizeof buf));
        return buf;
    }
    // asynchronous on the context's stream; out_dev is a DEVICE pointer (bytes, or 4-byte aligned RGBA pixels)
    void render(void *out_dev, size_t out_stride, size_t out_rows) { check(fr_plan_render(plan_, out_dev, out_stride, out_rows)); }
private:
    static int create(fr_ctx *c, fr_glyphset *gs, const fr_glyph_place_ex *p, const uint8_t *rgba, uint32_t n, const fr_text_run *r,
                      const uint8_t *clear, uint32_t nr, const fr_raster_params *prm, uint32_t flags, fr_plan **out)
    {
        return rgba ? fr_text_plan_create_rgba_ex(c, gs, p, rgba, n, r, clear, nr, prm, flags, out)
                    : fr_text_plan_create_ex(c, gs, p, n, r, nr, prm, flags, out);
    }
    static int create(fr_ctx *c, fr_glyphset *gs, const fr_glyph_place_affine *p, const uint8_t *rgba, uint32_t n, const fr_text_run *r,
                      const uint8_t *clear, uint32_t nr, const fr_raster_params *prm, uint32_t flags, fr_plan **out)
    {
        return rgba ? fr_text_plan_create_rgba_affine(c, gs, p, rgba, n, r, clear, nr, prm, flags, out)
                    : fr_text_plan_create_affine(c, gs, p, n, r, nr, prm, flags, out);
    }
    template <class PLACE>
    void init(Context &ctx, const std::vector<Glyph> &glyphs, const std::vector<PLACE> &places, const std::vector<fr_text_run> &runs,
              int samples_per_axis, uint32_t flags, const std::vector<uint8_t> *place_rgba, const std::vector<uint8_t> *run_clear_rgba)
    {
        std::vector<int16_t> pts, boxes;
        std::vector<uint32_t> cstart{0}, gstart{0};
        for (const Glyph &g : glyphs) {
            for (const Contour &c : g.contours) {
                for (const Point &p : c.points) { pts.push_back(p.x); pts.push_back(p.y); }
                cstart.push_back((uint32_t)(pts.size() / 2));
            }
            gstart.push_back((uint32_t)cstart.size() - 1);
            boxes.insert(boxes.end(), {g.box.x_min, g.box.y_min, g.box.x_max, g.box.y_max});
        }
        if (pts.empty()) pts.assign(2, 0);
        check(fr_glyphset_create(ctx.get(), pts.data(), cstart.data(), (uint32_t)cstart.size() - 1, gstart.data(),
                                 (uint32_t)glyphs.size(), &gs_));
        fr_raster_params prm{FR_COVERAGE_U8, samples_per_axis, FR_SAMPLE_CENTER, 0};
        int rc = fr_glyphset_set_boxes(gs_, boxes.data());
        if (rc == FR_OK)
            rc = create(ctx.get(), gs_, places.data(), place_rgba ? place_rgba->data() : nullptr, (uint32_t)places.size(), runs.data(),
                        run_clear_rgba ? run_clear_rgba->data() : nullptr, (uint32_t)runs.size(), &prm, flags, &plan_);
        if (rc != FR_OK) {
            fr_glyphset_destroy(gs_);
            gs_ = nullptr;
            check(rc);
        }
    }
    fr_glyphset *gs_ = nullptr;
    fr_plan *plan_ = nullptr;
};

}  // namespace fr_host

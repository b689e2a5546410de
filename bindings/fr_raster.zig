//! fr_raster.zig — Zig 0.15 binding of include/fr_raster.h for nyasyamorina/font-renderer.
//!
//! UNVERIFIED BY A COMPILER: no Zig toolchain exists in the build image (`zig version` -> not found), so
//! this file has never been compiled.  What IS checked (tests/test_abi.py::test_zig_binding_matches_the_header):
//! every function of the header is declared here with the same name, the same number of parameters and the
//! same integer / float / pointer widths, and the enums carry the header's values.  It is the binding a
//! maintainer drops into `src/tools/` next to the file it replaces (`src/tools/render_glyph.zig`); the C side
//! it declares is exercised by the Python / C++ hosts and the GPU parity tests.
//!
//! Drop-in contract: `renderGlyph` keeps the reference's signature
//!   pub fn renderGlyph(glyph: Glyph, font_info: Font.Information, font_size: u16) !Image.Gray
//! (src/tools/render_glyph.zig:11).  Memory stays with the reference's allocator: the image is
//! `Image.Gray.init` (src/tools/Image.zig:58-61, helpers.alloc) and the library only fills it.
const std = @import("std");

const Font = @import("../font/Font.zig");
const Glyph = @import("../font/Glyph.zig");
const Image = @import("Image.zig");
const Point = @import("geometry.zig").Point;

pub const fr_ctx = opaque {};
pub const fr_glyphset = opaque {};
pub const fr_plan = opaque {};
pub const fr_font = opaque {};

pub const Status = enum(c_int) { ok = 0, invalid = -1, hip = -2, nomem = -3, unsupported = -4 };
pub const Mode = enum(i32) { winding_i16 = 0, gray_debug = 1, mask_nonzero = 2, coverage_u8 = 3, sdf_u8 = 4 };
pub const SamplePhase = enum(i32) { corner = 0, center = 1 };
pub const FR_FONT_ALLOW_HINTED: u32 = 1;
/// crossing-rule flag of the _ex entry points (fr_raster.h: FR_FILL_CONSISTENT)
pub const FR_FILL_CONSISTENT: u32 = 1;
/// flags of fr_text_plan_create_rgba only (fr_raster.h): blend and resolve in linear light (sRGB framebuffer), B G R A output
pub const FR_TEXT_BGRA: u32 = 4;
pub const FR_TEXT_SRGB: u32 = 8;
/// flag of fr_text_plan_create_rgba only (fr_raster.h): draw over the pixels already in the output
pub const FR_TEXT_LOAD: u32 = 32;
/// flag of the four upright and _ex text plan entry points (fr_raster.h): rasterise each distinct glyph image once per render
pub const FR_TEXT_CACHE: u32 = 128;
/// flag of the RGBA text plan entry points (fr_raster.h): source-over alpha, a premultiplied output
pub const FR_TEXT_OVER: u32 = 256;
/// flag of the two _affine text plan entry points (fr_raster.h): FR_TEXT_CACHE for the matrix form, keyed by the bits of m
pub const FR_TEXT_CACHE_AFFINE: u32 = 512;
/// the flag space of fr_layer_over, fr_layer_shadow, fr_layer_outline, fr_layer_rects, fr_layer_paint and fr_layer_lcd (fr_raster.h): composite in linear light
pub const FR_LAYER_SRGB: u32 = 1;
/// fr_layer_lcd alone, beside FR_LAYER_SRGB: memory byte b takes sub-pixel 2 - b (a B G R panel); the other layer calls refuse it
pub const FR_LCD_BGR: u32 = 2;
/// the length of fr_layer_lcd's filter
pub const FR_LCD_TAPS = 5;
/// fr_layer_mask alone, beside FR_LAYER_SRGB: the mask is a plane of 1-byte elements (a coverage plan's output), any alignment
pub const FR_MASK_PLANE: u32 = 4;
/// fr_layer_mask alone: no layer, the destination is multiplied by 255 - t (destination-out)
pub const FR_MASK_ERASE: u32 = 8;
/// the modes of fr_layer_blend (fr_raster.h); FR_BLEND_MODES is their number
pub const FR_BLEND_MULTIPLY: u32 = 0;
pub const FR_BLEND_SCREEN: u32 = 1;
pub const FR_BLEND_OVERLAY: u32 = 2;
pub const FR_BLEND_DARKEN: u32 = 3;
pub const FR_BLEND_LIGHTEN: u32 = 4;
pub const FR_BLEND_HARD_LIGHT: u32 = 5;
pub const FR_BLEND_DIFFERENCE: u32 = 6;
pub const FR_BLEND_EXCLUSION: u32 = 7;
pub const FR_BLEND_PLUS: u32 = 8;
pub const FR_BLEND_MODES: u32 = 9;
/// LayerPaintParams.kind and .spread (fr_raster.h: fr_layer_paint)
pub const FR_GRADIENT_LINEAR: u32 = 0;
pub const FR_GRADIENT_RADIAL: u32 = 1;
pub const FR_SPREAD_PAD: u32 = 0;
pub const FR_SPREAD_REPEAT: u32 = 1;
pub const FR_SPREAD_REFLECT: u32 = 2;
pub const FR_GRADIENT_MAX_STOPS = 8;

pub const RasterParams = extern struct {
    mode: i32,
    samples_per_axis: i32,
    sample_phase: i32,
    reserved: i32 = 0,
};

pub const Job = extern struct {
    glyph: u32,
    min_x: i32,
    max_y: i32,
    w: u32,
    h: u32,
    out_x: u32,
    out_y: u32,
    scale: f32,
};

/// text runs (fr_raster.h: fr_glyph_place / fr_text_run; DESIGN.md section 5): a glyph at a pen position in 1/64 pixel
/// and a baseline row — what Appli.addChar / getTransform place (src/Appli.zig:318-349) —, and a run that composites
/// places[first .. first+count) into one w x h image at (out_x, out_y)
pub const GlyphPlace = extern struct {
    glyph: u32,
    pen_x64: i32,
    pen_y: i32,
};

/// a placement with its own size, slant and a baseline kept to 1/64 pixel (fr_raster.h: fr_glyph_place_ex): scale 0 is the
/// run's scale; slant k draws a point (x, y) of the outline at (x + k*y, y); pen_y64 = 64 * pen_y is row pen_y
pub const GlyphPlaceEx = extern struct {
    glyph: u32,
    pen_x64: i32,
    pen_y64: i32,
    scale: f32,
    slant: f32,
};

/// a placement with a 2 x 2 matrix (fr_raster.h: fr_glyph_place_affine): m = xx, xy, yx, yy draws the font-unit point
/// (x, y), y up, xx*x + xy*y pixels right of and yx*x + yy*y pixels above the pen; rotated, mirrored and sheared text
pub const GlyphPlaceAffine = extern struct {
    glyph: u32,
    pen_x64: i32,
    pen_y64: i32,
    m: [4]f32,
};

/// one rectangle of a layer and where it lands (fr_layer_over)
pub const LayerBlit = extern struct {
    src_x: u32,
    src_y: u32,
    w: u32,
    h: u32,
    dst_x: i32,
    dst_y: i32,
    opacity: u32,
};

/// the parameters of fr_layer_shadow: the layer's window, the destination rectangle, the offset, the stages and the colour
pub const LayerShadowParams = extern struct {
    src_x: u32,
    src_y: u32,
    w: u32,
    h: u32,
    dst_x: u32,
    dst_y: u32,
    dst_w: u32,
    dst_h: u32,
    dx: i32,
    dy: i32,
    spread: u32,
    blur_radius: u32,
    blur_passes: u32,
    rgba: [4]u8,
};

/// fr_layer_outline_params.kind: the grown shape, grown minus the layer, the layer minus its shrunk shape, the shrunk shape
pub const FR_OUTLINE_GROW: u32 = 0;
pub const FR_OUTLINE_RING: u32 = 1;
pub const FR_OUTLINE_INNER: u32 = 2;
pub const FR_OUTLINE_SHRINK: u32 = 3;
/// the largest fr_layer_outline_params.radius, in 1/16 pixel
pub const FR_OUTLINE_MAX_RADIUS: u32 = 256;

/// the parameters of fr_layer_outline: the layer's window, the destination rectangle, the offset, the radius in 1/16 pixel, the kind and the colour
pub const LayerOutlineParams = extern struct {
    src_x: u32,
    src_y: u32,
    w: u32,
    h: u32,
    dst_x: u32,
    dst_y: u32,
    dst_w: u32,
    dst_h: u32,
    dx: i32,
    dy: i32,
    radius: u32,
    kind: u32,
    rgba: [4]u8,
};

/// one anti-aliased rectangle of fr_layer_rects: edges in 1/64 pixel of the destination, y down, and a straight colour
pub const LayerRect = extern struct {
    x0: i32,
    y0: i32,
    x1: i32,
    y1: i32,
    rgba: [4]u8,
};

/// one colour stop of a gradient (fr_layer_paint): offset in 0 .. 65536, not below the stop before it, and a straight colour
pub const GradientStop = extern struct {
    offset: u32,
    rgba: [4]u8,
};

/// the parameters of fr_layer_paint: the layer's window, where it lands, and the gradient (geometry in 1/64 pixel of the
/// destination, y down; linear: (x0, y0) to (x1, y1); radial: centre (x0, y0), radius x1, y1 = 0)
pub const LayerPaintParams = extern struct {
    src_x: u32,
    src_y: u32,
    w: u32,
    h: u32,
    dst_x: i32,
    dst_y: i32,
    kind: u32,
    spread: u32,
    x0: i32,
    y0: i32,
    x1: i32,
    y1: i32,
    n_stops: u32,
    stops: [FR_GRADIENT_MAX_STOPS]GradientStop,
};

/// one window of fr_layer_lcd's coverage plane and where it lands: src_x in plane elements (three per pixel), w and h in
/// destination pixels, the text colour straight
pub const LcdBlit = extern struct {
    src_x: u32,
    src_y: u32,
    w: u32,
    h: u32,
    dst_x: i32,
    dst_y: i32,
    rgba: [4]u8,
};

/// one blit of fr_layer_warp: the window of the layer that is sampled, the rectangle of the image it owns, and the inverse
/// map (rectangle pixel to window position, 1/65536 pixel): u0, v0 at the centre of rectangle pixel (0, 0), (ux, vx) per
/// column and (uy, vy) per row; the opacity in 0 .. 255; reserved must be 0
pub const LayerWarpBlit = extern struct {
    src_x: u32,
    src_y: u32,
    w: u32,
    h: u32,
    dst_x: i32,
    dst_y: i32,
    dst_w: u32,
    dst_h: u32,
    u0: i64,
    v0: i64,
    ux: i32,
    uy: i32,
    vx: i32,
    vy: i32,
    opacity: u32,
    reserved: u32,
};

/// one rectangle of fr_layer_mask: where it lies in the layer (not used when erasing), where it lands, the mask element over
/// its top-left pixel, the opacity in 0 .. 255 and whether the mask is complemented (0 or 1)
pub const LayerMaskBlit = extern struct {
    src_x: u32,
    src_y: u32,
    w: u32,
    h: u32,
    dst_x: i32,
    dst_y: i32,
    mask_x: u32,
    mask_y: u32,
    opacity: u32,
    invert: u32,
};

/// fr_font_line_metrics: hhea, post and OS/2 in font units, y up; present bit 0: post, bit 1: OS/2
pub const FontLine = extern struct {
    ascender: i16,
    descender: i16,
    line_gap: i16,
    underline_position: i16,
    underline_thickness: i16,
    strikeout_size: i16,
    strikeout_position: i16,
    present: u16,
};

/// the kinds of fr_text_decoration
pub const FR_DECOR_UNDERLINE: u32 = 0;
pub const FR_DECOR_STRIKEOUT: u32 = 1;
pub const FR_DECOR_LINE_BOX: u32 = 2;

pub const TextRun = extern struct {
    first: u32,
    count: u32,
    w: u32,
    h: u32,
    out_x: u32,
    out_y: u32,
    scale: f32,
};

// ---- library / context
pub extern "c" fn fr_abi_version() c_int;
pub extern "c" fn fr_last_error() [*:0]const u8;
pub extern "c" fn fr_build_id() [*:0]const u8;
pub extern "c" fn fr_ctx_create(device: c_int, hip_stream: ?*anyopaque, out: *?*fr_ctx) c_int;
pub extern "c" fn fr_ctx_destroy(ctx: ?*fr_ctx) void;
pub extern "c" fn fr_ctx_sync(ctx: *fr_ctx) c_int;
pub extern "c" fn fr_ctx_set_option(ctx: *fr_ctx, key: [*:0]const u8, value: i64) c_int;
// ---- glyph sets
pub extern "c" fn fr_glyphset_create(ctx: *fr_ctx, points_xy: [*]const i16, contour_start: [*]const u32, n_contours: u32, glyph_start: [*]const u32, n_glyphs: u32, out: *?*fr_glyphset) c_int;
pub extern "c" fn fr_glyphset_destroy(gs: ?*fr_glyphset) void;
pub extern "c" fn fr_glyphset_prepare(gs: *fr_glyphset) c_int;
pub extern "c" fn fr_glyphset_stats(gs: *const fr_glyphset, n_segments: ?*u64, n_records: ?*u64) c_int;
pub extern "c" fn fr_glyphset_set_boxes(gs: *fr_glyphset, boxes: [*]const i16) c_int;
// ---- batched rasterization
pub extern "c" fn fr_plan_create(ctx: *fr_ctx, gs: *const fr_glyphset, jobs: [*]const Job, n_jobs: u32, params: *const RasterParams, out: *?*fr_plan) c_int;
pub extern "c" fn fr_plan_create_ex(ctx: *fr_ctx, gs: *const fr_glyphset, jobs: [*]const Job, n_jobs: u32, params: *const RasterParams, flags: u32, out: *?*fr_plan) c_int;
pub extern "c" fn fr_plan_destroy(plan: ?*fr_plan) void;
pub extern "c" fn fr_plan_render(plan: *fr_plan, out_dev: *anyopaque, out_stride: usize, out_rows: usize) c_int;
pub extern "c" fn fr_plan_render_timed(plan: *fr_plan, out_dev: *anyopaque, out_stride: usize, out_rows: usize, ms: *f32) c_int;
pub extern "c" fn fr_plan_pixels(plan: *const fr_plan) u64;
pub extern "c" fn fr_plan_stats(plan: *const fr_plan, n_jobs_cov4: ?*u32, n_jobs_general: ?*u32) c_int;
pub extern "c" fn fr_plan_describe(plan: *const fr_plan, buf: [*]u8, cap: usize) c_int;
pub extern "c" fn fr_text_plan_create(ctx: *fr_ctx, gs: *const fr_glyphset, places: [*]const GlyphPlace, n_places: u32, runs: [*]const TextRun, n_runs: u32, params: *const RasterParams, flags: u32, out: *?*fr_plan) c_int;
/// RGBA text plans (DESIGN.md section 5): place_rgba = 4 bytes (R, G, B, A) per placement, run_clear_rgba = 4 per run;
/// the plan renders RGBA pixels (4-byte aligned output, strides in pixels)
pub extern "c" fn fr_text_plan_create_rgba(ctx: *fr_ctx, gs: *const fr_glyphset, places: [*]const GlyphPlace, place_rgba: [*]const u8, n_places: u32, runs: [*]const TextRun, run_clear_rgba: [*]const u8, n_runs: u32, params: *const RasterParams, flags: u32, out: *?*fr_plan) c_int;
/// the two text plan entry points for GlyphPlaceEx placements (same runs, flags, colours and error codes)
pub extern "c" fn fr_text_plan_create_ex(ctx: *fr_ctx, gs: *const fr_glyphset, places: [*]const GlyphPlaceEx, n_places: u32, runs: [*]const TextRun, n_runs: u32, params: *const RasterParams, flags: u32, out: *?*fr_plan) c_int;
pub extern "c" fn fr_text_plan_create_rgba_ex(ctx: *fr_ctx, gs: *const fr_glyphset, places: [*]const GlyphPlaceEx, place_rgba: [*]const u8, n_places: u32, runs: [*]const TextRun, run_clear_rgba: [*]const u8, n_runs: u32, params: *const RasterParams, flags: u32, out: *?*fr_plan) c_int;
/// the same two for GlyphPlaceAffine placements (the text_affine_* kernels)
pub extern "c" fn fr_text_plan_create_affine(ctx: *fr_ctx, gs: *const fr_glyphset, places: [*]const GlyphPlaceAffine, n_places: u32, runs: [*]const TextRun, n_runs: u32, params: *const RasterParams, flags: u32, out: *?*fr_plan) c_int;
pub extern "c" fn fr_text_plan_create_rgba_affine(ctx: *fr_ctx, gs: *const fr_glyphset, places: [*]const GlyphPlaceAffine, place_rgba: [*]const u8, n_places: u32, runs: [*]const TextRun, run_clear_rgba: [*]const u8, n_runs: u32, params: *const RasterParams, flags: u32, out: *?*fr_plan) c_int;
pub extern "c" fn fr_allgather_bands(ctx: *fr_ctx, nccl_comm: *anyopaque, atlas_dev: *anyopaque, band_bytes: usize) c_int;
pub extern "c" fn fr_gather_bands(ctx: *fr_ctx, nccl_comm: *anyopaque, atlas_dev: *anyopaque, band_bytes: usize, root: c_int) c_int;
pub extern "c" fn fr_render_batch(ctx: *fr_ctx, gs: *const fr_glyphset, jobs: [*]const Job, n_jobs: u32, params: *const RasterParams, out_host: *anyopaque, out_stride: usize, out_rows: usize) c_int;
pub extern "c" fn fr_render_batch_ex(ctx: *fr_ctx, gs: *const fr_glyphset, jobs: [*]const Job, n_jobs: u32, params: *const RasterParams, flags: u32, out_host: *anyopaque, out_stride: usize, out_rows: usize) c_int;
// ---- renderGlyph drop-in
pub extern "c" fn fr_render_glyph_dims(box: *const [4]i16, units_per_em: u16, font_size: u16, min_corner: *[2]i16, max_corner: *[2]i16, width: *u16, height: *u16, scale: ?*f32) c_int;
pub extern "c" fn fr_render_glyph(ctx: *fr_ctx, points_xy: [*]const i16, contour_start: [*]const u32, n_contours: u32, box: *const [4]i16, units_per_em: u16, font_size: u16, mode: i32, out_host: *anyopaque) c_int;
pub extern "c" fn fr_render_glyph_ex(ctx: *fr_ctx, points_xy: [*]const i16, contour_start: [*]const u32, n_contours: u32, box: *const [4]i16, units_per_em: u16, font_size: u16, mode: i32, flags: u32, out_host: *anyopaque) c_int;
// ---- exact-integer path
pub extern "c" fn fr_glyph_info_init(ctx: *fr_ctx, points_xy: [*]const i16, contour_start: [*]const u32, n_contours: u32, curve_type: [*]u8, include_p0: [*]u8) c_int;
pub extern "c" fn fr_winding_in_glyph(ctx: *fr_ctx, points_xy: [*]const i16, contour_start: [*]const u32, n_contours: u32, query_xy: [*]const i16, n_query: u32, out_winding: [*]i16) c_int;
pub extern "c" fn fr_winding_lattice(ctx: *fr_ctx, points_xy: [*]const i16, contour_start: [*]const u32, n_contours: u32, box: *const [4]i16, out_host: [*]i16) c_int;
pub extern "c" fn fr_glyph_debug_render(ctx: *fr_ctx, points_xy: [*]const i16, contour_start: [*]const u32, n_contours: u32, box: *const [4]i16, winding_scale: u8, rgb_host: [*]u8) c_int;
// build-defined (no reference counterpart): the exact-integer path on a K-times refined lattice
pub extern "c" fn fr_exact_lattice(ctx: *fr_ctx, points_xy: [*]const i16, contour_start: [*]const u32, n_contours: u32, k: u32, x0: i32, y0: i32, w: u32, h: u32, out_host: [*]i16) c_int;
pub extern "c" fn fr_exact_coverage(ctx: *fr_ctx, points_xy: [*]const i16, contour_start: [*]const u32, n_contours: u32, k: u32, x0: i32, y0: i32, w_px: u32, h_px: u32, n: u32, out_host: [*]u8) c_int;
// ---- atlas layout (host side)
pub extern "c" fn fr_atlas_layout(boxes: [*]const i16, n_glyphs: u32, first_glyph: u32, units_per_em: [*]const u16, n_upm: u32, font_size: u16, cell: u32, cols: u32, rows_per_page: u32, jobs_out: [*]Job, page_of_job: ?[*]u32, n_pages: ?*u32) c_int;
pub extern "c" fn fr_atlas_layout_glyph_dims(boxes: [*]const i16, n_glyphs: u32, first_glyph: u32, units_per_em: [*]const u16, n_upm: u32, font_size: u16, atlas_w: u32, @"align": u32, jobs_out: [*]Job, atlas_h: ?*u32) c_int;
// ---- contour producer (host side; the Zig host has font/Font.zig and does not need it)
pub extern "c" fn fr_font_open(ttf_bytes: *const anyopaque, len: usize, flags: u32, out: *?*fr_font) c_int;
pub extern "c" fn fr_font_close(font: ?*fr_font) void;
pub extern "c" fn fr_font_info(font: *const fr_font, units_per_em: ?*u16, num_glyphs: ?*u16, y0_baseline: ?*c_int) c_int;
pub extern "c" fn fr_font_char_to_glyph(font: *const fr_font, codepoint: u32, glyph_index: *u16) c_int;
pub extern "c" fn fr_font_glyph_advance(font: *const fr_font, glyph_index: u16, advance_width: *i16) c_int;
pub extern "c" fn fr_text_layout(font: *const fr_font, codepoints: [*]const u32, n: u32, font_size: u16, glyph_index_out: [*]u16, pen_x64_out: [*]i32, end_pen_x64: ?*i32) c_int;
/// where a line's decorations belong: the font's line metrics, and a decoration's rows below the baseline in 1/64 pixel
pub extern "c" fn fr_font_line_metrics(font: *const fr_font, out: *FontLine) c_int;
pub extern "c" fn fr_text_decoration(font: *const fr_font, font_size: u16, kind: u32, top_y64: *i32, bottom_y64: *i32) c_int;
pub extern "c" fn fr_font_glyph_measure(font: *fr_font, glyph_index: u16, n_contours: *u32, n_points: *u32, box: *[4]i16) c_int;
pub extern "c" fn fr_font_glyph_fill(font: *fr_font, glyph_index: u16, points_xy: [*]i16, contour_start: [*]u32) c_int;
// ---- QOI writer (host side; byte-compatible with tools/qoi.zig, which the Zig host keeps)
pub extern "c" fn fr_qoi_bound(width: u32, height: u32) usize;
pub extern "c" fn fr_qoi_encode_rgb(rgb: [*]const u8, width: u32, height: u32, out: [*]u8, cap: usize, n_out: *usize) c_int;
pub extern "c" fn fr_qoi_encode_gray(gray: [*]const u8, width: u32, height: u32, stride: usize, out: [*]u8, cap: usize, n_out: *usize) c_int;
/// a standard 4-channel QOI stream (the QOI specification; tools/qoi.zig writes RGB only)
pub extern "c" fn fr_qoi_encode_rgba(rgba: [*]const u8, width: u32, height: u32, stride_px: usize, out: [*]u8, cap: usize, n_out: *usize) c_int;
/// the sRGB conversions of FR_TEXT_SRGB plans: 8-bit sRGB -> 16-bit linear light, and back (rounded in the encoded domain)
pub extern "c" fn fr_srgb_decode(in: [*]const u8, n: usize, out: [*]u16) c_int;
pub extern "c" fn fr_srgb_encode(in: [*]const u16, n: usize, out: [*]u8) c_int;
/// premultiplied -> straight alpha in place (the output of FR_TEXT_OVER plans); srgb != 0: in linear light
pub extern "c" fn fr_rgba_unpremultiply(rgba: [*]u8, n_pixels: usize, srgb: c_int) c_int;
/// rectangles of a premultiplied layer over a premultiplied image, both in device memory, at whole-pixel offsets and an opacity
pub extern "c" fn fr_layer_over(ctx: *Ctx, src_dev: *const anyopaque, src_stride_px: usize, src_rows: usize, dst_dev: *anyopaque, dst_stride_px: usize, dst_rows: usize, blits: ?[*]const LayerBlit, n_blits: u32, flags: u32) c_int;
/// fr_rgba_unpremultiply on the device, over a w x h window of an image in rows of stride_px pixels
pub extern "c" fn fr_layer_unpremultiply(ctx: *Ctx, rgba_dev: *anyopaque, stride_px: usize, w: u32, h: u32, srgb: c_int) c_int;
/// the alpha of a layer's window, spread, box-blurred, moved and tinted: a premultiplied layer written over a rectangle of the destination
pub extern "c" fn fr_layer_shadow(ctx: *Ctx, src_dev: *const anyopaque, src_stride_px: usize, src_rows: usize, dst_dev: *anyopaque, dst_stride_px: usize, dst_rows: usize, shadow: *const LayerShadowParams, flags: u32) c_int;
/// the alpha of a layer's window grown or shrunk by a disc, combined with the layer by the kind, moved and tinted: a premultiplied layer written over a rectangle of the destination
pub extern "c" fn fr_layer_outline(ctx: *Ctx, src_dev: *const anyopaque, src_stride_px: usize, src_rows: usize, dst_dev: *anyopaque, dst_stride_px: usize, dst_rows: usize, outline: *const LayerOutlineParams, flags: u32) c_int;
/// anti-aliased rectangles, each in one straight colour, composited in order over a premultiplied image in device memory
pub extern "c" fn fr_layer_rects(ctx: *Ctx, dst_dev: *anyopaque, dst_stride_px: usize, dst_rows: usize, rects: ?[*]const LayerRect, n_rects: u32, flags: u32) c_int;
/// a linear or radial gradient composited over a premultiplied image through the alpha of a layer's window (src_dev null: full coverage)
pub extern "c" fn fr_layer_paint(ctx: *Ctx, src_dev: ?*const anyopaque, src_stride_px: usize, src_rows: usize, dst_dev: *anyopaque, dst_stride_px: usize, dst_rows: usize, paint: *const LayerPaintParams, flags: u32) c_int;
/// sub-pixel (LCD) text: windows of a 3x-wide coverage plane filtered across sub-pixels (weights: FR_LCD_TAPS values adding up to 256, null: the default) and composited with an alpha per colour byte
pub extern "c" fn fr_layer_lcd(ctx: *Ctx, cov_dev: *const anyopaque, cov_stride: usize, cov_rows: usize, dst_dev: *anyopaque, dst_stride_px: usize, dst_rows: usize, blits: ?[*]const LcdBlit, n_blits: u32, weights: ?*const [FR_LCD_TAPS]u16, flags: u32) c_int;
/// rectangles of a premultiplied layer over a premultiplied image at an opacity per pixel taken from a mask (a layer's alpha, or with FR_MASK_PLANE a plane of bytes); with FR_MASK_ERASE (src_dev null) the mask lowers the image instead
pub extern "c" fn fr_layer_mask(ctx: *Ctx, src_dev: ?*const anyopaque, src_stride_px: usize, src_rows: usize, mask_dev: *const anyopaque, mask_stride: usize, mask_rows: usize, dst_dev: *anyopaque, dst_stride_px: usize, dst_rows: usize, blits: ?[*]const LayerMaskBlit, n_blits: u32, flags: u32) c_int;
/// windows of a premultiplied layer over a premultiplied image through an affine map each (scaled, turned, moved by a fraction of a pixel), sampled bilinearly in exact integers
pub extern "c" fn fr_layer_warp(ctx: *Ctx, src_dev: *const anyopaque, src_stride_px: usize, src_rows: usize, dst_dev: *anyopaque, dst_stride_px: usize, dst_rows: usize, blits: ?[*]const LayerWarpBlit, n_blits: u32, flags: u32) c_int;
/// fr_layer_over with a separable blend mode (FR_BLEND_*) in the place of source-over, one mode per call, in exact integers with one rounding
pub extern "c" fn fr_layer_blend(ctx: *Ctx, src_dev: *const anyopaque, src_stride_px: usize, src_rows: usize, dst_dev: *anyopaque, dst_stride_px: usize, dst_rows: usize, blits: ?[*]const LayerBlit, n_blits: u32, mode: u32, flags: u32) c_int;
// ---- self-tests of the two arithmetic shortcuts (device-side, exhaustive)
pub extern "c" fn fr_selftest_division(d_lo: u32, d_hi: u32, mismatches: *u64, bad_divisor: ?*u32, bad_x_bits: ?*u32) c_int;
pub extern "c" fn fr_selftest_sqrt(mismatches: *u64, bad_x_bits: ?*u32) c_int;
pub extern "c" fn fr_selftest_row_cuts(gs: *fr_glyphset, jobs: [*]const Job, n_jobs: u32, samples_per_axis: c_int, phase: c_int, pairs: *u64, mismatches: *u64, first_bad: ?*[3]u32) c_int;
pub extern "c" fn fr_selftest_cand_records(gs: *fr_glyphset, live: *u64, mismatches: *u64, first_bad: ?*[2]u32, glyph_live: ?[*]u32) c_int;

pub const Error = error{ RasterFailed, OutOfMemory };

var g_ctx: ?*fr_ctx = null;

fn context() Error!*fr_ctx {
    if (g_ctx == null) {
        if (fr_ctx_create(0, null, &g_ctx) != 0) return error.RasterFailed;
    }
    return g_ctx.?;
}

/// Releases the process-wide context (its stream, device arena and pinned staging block).  Call once from the
/// host's shutdown path, next to Font.deinit (src/main.zig:33); a later renderGlyph creates a fresh one.
pub fn deinit() void {
    if (g_ctx) |c| fr_ctx_destroy(c);
    g_ctx = null;
}

/// Flat view of a Glyph: every contour's points live in ONE allocation in contour order
/// (src/font/Glyph.zig:89-96), and Point(i16) is an extern struct {x, y} (geometry.zig:7-11),
/// so `contours[0].points.ptr` is already the i16 (x,y) array the C ABI wants — no copy.
/// Only the contour offsets are built here.
fn flatten(glyph: Glyph, starts: []u32) [*]const i16 {
    starts[0] = 0;
    for (glyph.contours, 0..) |contour, i| starts[i + 1] = starts[i] + @as(u32, @intCast(contour.points.len));
    if (glyph.contours.len == 0) return @ptrCast(&[_]i16{ 0, 0 });
    return @ptrCast(glyph.contours[0].points.ptr);
}

fn boxOf(glyph: Glyph) [4]i16 {
    return .{ glyph.box.x_min, glyph.box.y_min, glyph.box.x_max, glyph.box.y_max };
}

/// Drop-in for src/tools/render_glyph.zig:11 — same signature, same bytes.
pub fn renderGlyph(glyph: Glyph, font_info: Font.Information, font_size: u16) !Image.Gray {
    const helpers = @import("../helpers.zig");
    const ctx = try context();
    const box = boxOf(glyph);
    var mn: [2]i16 = undefined;
    var mx: [2]i16 = undefined;
    var w: u16 = 0;
    var h: u16 = 0;
    if (fr_render_glyph_dims(&box, font_info.units_per_em, font_size, &mn, &mx, &w, &h, null) != 0) return error.RasterFailed;

    var im: Image.Gray = .init(w, h); // render_glyph.zig:22 — the caller's allocator owns the pixels
    errdefer im.deinit();

    const starts = helpers.alloc(u32, glyph.contours.len + 1);
    defer helpers.allocator.free(starts);
    const pts = flatten(glyph, starts);
    const rc = fr_render_glyph(ctx, pts, starts.ptr, @intCast(glyph.contours.len), &box, font_info.units_per_em, font_size, @intFromEnum(Mode.gray_debug), im.data.ptr);
    if (rc != 0) return error.RasterFailed;
    return im;
}

/// The same grid as renderGlyph, holding the winding numbers themselves: Image.Winding
/// (src/tools/Image.zig:85-130; `scaler` / `overflow_color` are the display parameters of its colour map).
pub fn renderGlyphWinding(glyph: Glyph, font_info: Font.Information, font_size: u16, scaler: u8, overflow_color: u8) !Image.Winding {
    const helpers = @import("../helpers.zig");
    const ctx = try context();
    const box = boxOf(glyph);
    var mn: [2]i16 = undefined;
    var mx: [2]i16 = undefined;
    var w: u16 = 0;
    var h: u16 = 0;
    if (fr_render_glyph_dims(&box, font_info.units_per_em, font_size, &mn, &mx, &w, &h, null) != 0) return error.RasterFailed;

    var im: Image.Winding = .init(w, h, scaler, overflow_color); // Image.zig:101-104
    errdefer im.deinit();

    const starts = helpers.alloc(u32, glyph.contours.len + 1);
    defer helpers.allocator.free(starts);
    const pts = flatten(glyph, starts);
    const rc = fr_render_glyph(ctx, pts, starts.ptr, @intCast(glyph.contours.len), &box, font_info.units_per_em, font_size, @intFromEnum(Mode.winding_i16), im.data.ptr);
    if (rc != 0) return error.RasterFailed;
    return im;
}

/// Image.GlyphDebug.render's lattice (src/tools/Image.zig:227-236) through the exact-integer
/// path: fills `out` ((x_max-x_min+3) * (y_max-y_min+3) i16) with windingInGlyph values.
pub fn windingLattice(glyph: Glyph, out: []i16) !void {
    const helpers = @import("../helpers.zig");
    const ctx = try context();
    const box = boxOf(glyph);
    const starts = helpers.alloc(u32, glyph.contours.len + 1);
    defer helpers.allocator.free(starts);
    const pts = flatten(glyph, starts);
    if (fr_winding_lattice(ctx, pts, starts.ptr, @intCast(glyph.contours.len), &box, out.ptr) != 0) return error.RasterFailed;
}

/// Drop-in for Image.GlyphDebug.render (src/tools/Image.zig:220-240): the coloured lattice with the glyph's points
/// marked, written into the Image.RGB the reference's own init allocates (Image.zig:181-190).
pub fn glyphDebugRender(glyph: Glyph, winding_scale: u8) !Image.GlyphDebug {
    const helpers = @import("../helpers.zig");
    const ctx = try context();
    const box = boxOf(glyph);
    var im: Image.GlyphDebug = .init(glyph.box, winding_scale, 150, .{ 255, 255, 0 }, .{ 0, 255, 255 });
    errdefer im.rgb.deinit();
    const starts = helpers.alloc(u32, glyph.contours.len + 1);
    defer helpers.allocator.free(starts);
    const pts = flatten(glyph, starts);
    if (fr_glyph_debug_render(ctx, pts, starts.ptr, @intCast(glyph.contours.len), &box, winding_scale, @ptrCast(im.rgb.data.ptr)) != 0) return error.RasterFailed;
    return im;
}

/// A batch of glyphs into one atlas page (build-defined cell grid: fr_atlas_layout): `glyphs` are flattened into
/// one points array (one copy — they live in separate allocations of Font.glyphs), rendered as n x n-sample
/// coverage into a `cols * cell` wide Image.Gray of ceil(len / cols) cell rows.
pub fn renderAtlas(glyphs: []const Glyph, font_info: Font.Information, font_size: u16, cell: u32, cols: u32, samples_per_axis: i32) !Image.Gray {
    const helpers = @import("../helpers.zig");
    const ctx = try context();
    var n_points: usize = 0;
    var n_contours: usize = 0;
    for (glyphs) |g| {
        n_contours += g.contours.len;
        for (g.contours) |c| n_points += c.points.len;
    }
    const pts = helpers.alloc(i16, 2 * @max(n_points, 1));
    defer helpers.allocator.free(pts);
    const cstart = helpers.alloc(u32, n_contours + 1);
    defer helpers.allocator.free(cstart);
    const gstart = helpers.alloc(u32, glyphs.len + 1);
    defer helpers.allocator.free(gstart);
    const boxes = helpers.alloc(i16, 4 * @max(glyphs.len, 1));
    defer helpers.allocator.free(boxes);
    var p: usize = 0;
    var c_i: usize = 0;
    cstart[0] = 0;
    gstart[0] = 0;
    for (glyphs, 0..) |g, gi| {
        for (g.contours) |c| {
            for (c.points) |pt| {
                pts[2 * p] = pt.x;
                pts[2 * p + 1] = pt.y;
                p += 1;
            }
            c_i += 1;
            cstart[c_i] = @intCast(p);
        }
        gstart[gi + 1] = @intCast(c_i);
        const b = boxOf(g);
        @memcpy(boxes[4 * gi .. 4 * gi + 4], &b);
    }
    const jobs = helpers.alloc(Job, @max(glyphs.len, 1));
    defer helpers.allocator.free(jobs);
    const upm = [1]u16{font_info.units_per_em};
    if (fr_atlas_layout(boxes.ptr, @intCast(glyphs.len), 0, &upm, 1, font_size, cell, cols, 0, jobs.ptr, null, null) != 0) return error.RasterFailed;

    var gs: ?*fr_glyphset = null;
    if (fr_glyphset_create(ctx, pts.ptr, cstart.ptr, @intCast(n_contours), gstart.ptr, @intCast(glyphs.len), &gs) != 0) return error.RasterFailed;
    defer fr_glyphset_destroy(gs);

    const rows: u32 = @intCast((glyphs.len + cols - 1) / cols);
    var im: Image.Gray = .init(@intCast(cols * cell), @intCast(rows * cell));
    errdefer im.deinit();
    @memset(im.data, 0);
    const prm = RasterParams{ .mode = @intFromEnum(Mode.coverage_u8), .samples_per_axis = samples_per_axis, .sample_phase = @intFromEnum(SamplePhase.center) };
    if (fr_render_batch(ctx, gs.?, jobs.ptr, @intCast(glyphs.len), &prm, im.data.ptr, cols * cell, rows * cell) != 0) return error.RasterFailed;
    return im;
}

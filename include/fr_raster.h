/*
 * fr_raster.h — C ABI of the MI355X-native glyph rasterizer (libfr_raster.so).
 *
 * This is the drop-in boundary for ONE path of nyasyamorina/font-renderer: the
 * per-pixel winding / coverage loop of src/tools/render_glyph.zig (and the
 * TriangulatedGlyph + shader.slang + Vulkan pipeline that draws the same filled
 * region).  The host keeps the reference's Glyph (src/font/Glyph.zig:11-24) and
 * Image (src/tools/Image.zig:44-130) types; it hands this library flat views of
 * the glyph's contiguous i16 points and a caller-allocated output buffer.
 * Reference-side binding: see INTEGRATION.md and bindings/fr_raster.zig.
 *
 * Plain pointers and sizes only; no C++ / torch types.  All functions return an
 * fr_status (0 = ok, < 0 = error) unless noted; fr_last_error() returns a
 * thread-local message for the last failing call.  The library never frees or
 * retains host pointers past a call, never aborts and never throws across the
 * ABI.  One fr_ctx is used from one thread at a time (the reference is
 * single-threaded: SURVEY §8b).
 *
 * There is NO CPU fallback: every compute entry point runs hand-written HIP
 * kernels on a gfx950 device and fails with FR_E_HIP when none is usable.
 */
#ifndef FR_RASTER_H
#define FR_RASTER_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FR_ABI_VERSION 1

typedef enum fr_status {
    FR_OK = 0,
    FR_E_INVALID = -1,      /* bad argument / malformed glyph tables               */
    FR_E_HIP = -2,          /* HIP runtime error or no usable device               */
    FR_E_NOMEM = -3,        /* host or device allocation failed                    */
    FR_E_UNSUPPORTED = -4   /* valid request outside the implemented envelope      */
} fr_status;

/* What one output element holds.  The value maps are the reference's own:
 *   FR_WINDING_I16  int16 winding number at the sample      (Image.Winding.data, Image.zig:85-88;
 *                                                            glyphWindingAt, render_glyph.zig:35-73)
 *   FR_GRAY_DEBUG   u8 clamp(w*20+100, 0, 255)               (render_glyph.zig:28 — what renderGlyph emits)
 *   FR_MASK_NONZERO u8 (w != 0) ? 255 : 0                    (render_glyph.zig:29, the commented alternative)
 *   FR_COVERAGE_U8  u8 round(255*k/n^2), k = # of the n x n sub-samples with w != 0
 *                   (non-zero fill as :29; box filter = the MSAA average resolve,
 *                    VulkanContext.zig:307-313 — the reference's only anti-aliasing)        */
typedef enum fr_mode {
    FR_WINDING_I16 = 0,
    FR_GRAY_DEBUG = 1,
    FR_MASK_NONZERO = 2,
    FR_COVERAGE_U8 = 3,
    FR_SDF_U8 = 4           /* BUILD-DEFINED (the reference has no SDF): u8 = clamp(round(128 + 16*d)),
                               d = distance in pixels from the sample to the nearest quadratic segment,
                               + inside (winding != 0) / - outside; n must be 1.  Exact definition:
                               font-renderer_amd/csrc/fr_sdf.hip                                         */
} fr_mode;

/* Sub-sample k of an axis sits at (k + phase)/n of a pixel:
 *   FR_SAMPLE_CORNER phase 0   — with n = 1 exactly the reference's sample, the pixel
 *                                *corner* (min_x + x, max_y - y) (render_glyph.zig:26-27)
 *   FR_SAMPLE_CENTER phase 1/2 — regular n x n grid centred in the pixel              */
typedef enum fr_sample_phase { FR_SAMPLE_CORNER = 0, FR_SAMPLE_CENTER = 1 } fr_sample_phase;

/* Crossing-rule flags of the _ex entry points (BUILD-DEFINED).  flags = 0 is the reference's rule —
 * bit for bit what the entry points without _ex compute; any bit not defined here is FR_E_INVALID.
 *   FR_FILL_CONSISTENT  the non-zero winding of the SAME sample points (cx, cy) (binary32 exactly as fr_job says) with a
 *       consistent crossing rule instead of the reference's root acceptance 0 <= t < 1 (render_glyph.zig:49-69, which
 *       counts false crossings on a ray through a vertex, an extremum or along a horizontal edge):
 *       1. pieces: a segment with a == 0 is one piece p0 -> p2 (none if p0y == p2y); a quadratic one is split at its
 *          y-extremum t_v = b / a (b = p0y - p1y) into its y-monotone halves (those with t in [0, 1]); a piece whose
 *          y-extent is a single value contributes nothing;
 *       2. a piece with exact end heights ylo < yhi (the integers p0y, p2y or the vertex height p0y - b^2 / a) is
 *          crossed by the ray at height cy iff ylo <= cy < yhi, decided exactly on cy as the binary32 it is;
 *       3. the crossing adds -1 if the piece rises along t, +1 if it falls;
 *       4. its abscissa xx is the reference's expression (:51 / :60-61 for t, :53 / :65 for xx) with delta clamped at 0
 *          before the square root, and it counts iff !(xx < cx), as in the reference.
 *       So a vertex the outline passes through is counted once, an extremum twice with opposite signs (or not at all),
 *       a horizontal edge never.  Every mode, n and phase; the exact-integer path (fr_exact_*, fr_winding_lattice,
 *       fr_glyph_debug_render) has no flags and stays the reference's.                                                  */
#define FR_FILL_CONSISTENT 1u

typedef struct fr_raster_params {
    int32_t mode;              /* fr_mode                                              */
    int32_t samples_per_axis;  /* n in {1,2,4}; must be 1 unless mode = FR_COVERAGE_U8  */
    int32_t sample_phase;      /* fr_sample_phase                                      */
    int32_t reserved;          /* 0                                                    */
} fr_raster_params;

/* One glyph cell to rasterize.  Sample point of pixel (x, y), sub-sample (i, j):
 *     cx = (f32(min_x + x) + (i + phase)/n) / scale
 *     cy = (f32(max_y - y) - (j + phase)/n) / scale        (render_glyph.zig:26-27: division,
 *                                                            y-down image, font-unit ray origin)
 * renderGlyph's own grid is min = floor(box_min*scale), max = ceil(box_max*scale),
 * w = max_x-min_x+1, h = max_y-min_y+1 (render_glyph.zig:13-19): fr_render_glyph_dims. */
typedef struct fr_job {
    uint32_t glyph;            /* index into the glyph set                             */
    int32_t  min_x, max_y;     /* pixel coordinate of column 0 / row 0                 */
    uint32_t w, h;             /* cell size in pixels                                  */
    uint32_t out_x, out_y;     /* destination of the cell's (0,0) in the output, elements / rows */
    float    scale;            /* font_size / units_per_em (render_glyph.zig:13)       */
} fr_job;

typedef struct fr_ctx fr_ctx;
typedef struct fr_glyphset fr_glyphset;
typedef struct fr_plan fr_plan;

/* ---- library / context -------------------------------------------------- */
int fr_abi_version(void);
const char *fr_last_error(void);
/* a string that changes whenever a source file of the library does: "r03-" + the first 12 hex digits of the SHA-256 of
 * csrc's sources, computed by the Makefile at build time (profiles/traffic.json is keyed by it) */
const char *fr_build_id(void);

/* device: HIP device ordinal.  hip_stream: a hipStream_t to launch on (e.g. the
 * caller's torch stream), or NULL to let the context create and own one.       */
int fr_ctx_create(int device, void *hip_stream, fr_ctx **out);
void fr_ctx_destroy(fr_ctx *ctx);
int fr_ctx_sync(fr_ctx *ctx);
/* tuning / test knobs: "kmax" (crossings kept per sample row, in registers, before the
 * exact direct-sum fallback: rounded up to 8, 16 or 32; default 32), "strip_px" (column
 * strip width in pixels, multiple of 16, <= 256: wider cells are rendered strip by strip; the fast kernels use
 * the largest of 64 / 128 / 256 that does not exceed it),
 * "cov4" (0: every job takes the general kernel), "row_cuts" (default 1: the set-up of the fast kernels reads the
 * class of a sample row off the glyph set's row cuts — two heights per candidate root, found once by
 * fr_glyphset_create, 16 bytes per segment; 0: it evaluates the reference's acceptance expression at the row, as
 * fr_render_glyph always does.  The pixels are the same either way: fr_selftest_row_cuts), "cand_records" (default 1, and only
 * with "row_cuts": that set-up also reads each candidate root's record — the coefficients, the reciprocal, the step codes,
 * its cut — ready-made from the glyph set's candidate table, built once by fr_glyphset_create, 96 bytes per segment,
 * live candidates first and in record order; 0: it builds every candidate from the segment's control points.  The same
 * records either way: fr_selftest_cand_records), "sdf_cull" (0: FR_SDF_U8 looks at every segment from
 * every pixel — the culls are exact, this is how the tests show it), "zero_copy" (1: fr_render_glyph renders small
 * glyphs straight from / into pinned host memory; measured no faster, off by default), "overlap" (a plan that needs several kernel launches forks the
 * smaller ones onto an internal second stream and joins them: 1 (default) for plans of >= 32 Mpixel — below that one
 * stream is quicker —, 2 always, 0 never), "graph" (1: the launches of a plan's render — fork and join included — are
 * captured into a hipGraph at the first fr_plan_render to a destination and replayed with one hipGraphLaunch afterwards;
 * captured again when the destination or an option changes.  Measured: worth 3 - 6 % on a plan of four
 * launches forked over two streams, a loss of ~5 us per render on plans of one to three launches; default 0), "min_wgs", "fuse_prepare", "lds_pad"   */
int fr_ctx_set_option(fr_ctx *ctx, const char *key, int64_t value);

/* ---- glyph sets: Glyph[] flattened (Glyph.zig:11-24) ---------------------
 * points_xy      : i16 (x,y) pairs, every contour of every glyph back to back — the
 *                  reference already keeps one glyph's points in one allocation
 *                  (Glyph.zig:89-96), so a single glyph is passed without copying;
 * contour_start  : n_contours+1 offsets (in points); contour c = [start[c], start[c+1]),
 *                  even index on-curve, odd index control, last == first (Glyph.zig:23),
 *                  so its length is odd and >= 3 (or 1: a degenerate contour, 0 curves);
 * glyph_start    : n_glyphs+1 offsets (in contours).
 * Uploads the points to HBM and runs the per-segment precompute kernel once
 * (root records with exact acceptance intervals).  Scale-independent:
 * one glyph set serves every font size, mode and sample count.                     */
int fr_glyphset_create(fr_ctx *ctx, const int16_t *points_xy, const uint32_t *contour_start,
                       uint32_t n_contours, const uint32_t *glyph_start, uint32_t n_glyphs,
                       fr_glyphset **out);
void fr_glyphset_destroy(fr_glyphset *gs);
/* re-runs the precompute kernel on the context's stream (asynchronous); for timing */
int fr_glyphset_prepare(fr_glyphset *gs);
/* totals, for reporting: segments (curves) and surviving root records */
int fr_glyphset_stats(const fr_glyphset *gs, uint64_t *n_segments, uint64_t *n_records);
/* the glyphs' boxes (Glyph.box: x_min, y_min, x_max, y_max per glyph, font units; n_glyphs x 4 i16), which text plans
 * size their instance cells from (fr_text_plan_create); copied, host side.  Until set, fr_text_plan_create fails.       */
int fr_glyphset_set_boxes(fr_glyphset *gs, const int16_t *boxes);

/* ---- batched rasterization ----------------------------------------------
 * A plan keeps the job table resident on the device so a batch can be re-rendered
 * without host traffic (atlas pages, benchmark steps).                              */
int fr_plan_create(fr_ctx *ctx, const fr_glyphset *gs, const fr_job *jobs, uint32_t n_jobs,
                   const fr_raster_params *params, fr_plan **out);
/* the same with crossing-rule flags (FR_FILL_CONSISTENT); fr_plan_create is flags = 0                                 */
int fr_plan_create_ex(fr_ctx *ctx, const fr_glyphset *gs, const fr_job *jobs, uint32_t n_jobs,
                      const fr_raster_params *params, uint32_t flags, fr_plan **out);
void fr_plan_destroy(fr_plan *plan);
/* Every render starts from the glyph POINTS (nothing derived is reused between renders): the render
 * kernels build the root records of a glyph of <= 128 (general kernel) / <= 768 (cov4 / win1 kernels) segments
 * themselves, in LDS ("fused", decided per job); the precompute kernel is re-run first for the larger glyphs only.
 * Asynchronous on the context's stream.  out_dev: DEVICE pointer to an array of
 * out_rows rows of out_stride elements (u8, or i16 for FR_WINDING_I16); every job
 * must fit inside it (checked); out_stride <= 2^26 elements (FR_E_INVALID beyond: the kernels address the rows of a
 * wave band by 32-bit offsets from the band's base).  Pixels outside all jobs are not touched.                     */
int fr_plan_render(fr_plan *plan, void *out_dev, size_t out_stride, size_t out_rows);
/* same, bracketed by HIP events on the launch stream; synchronous; *ms = kernel time */
int fr_plan_render_timed(fr_plan *plan, void *out_dev, size_t out_stride, size_t out_rows, float *ms);
uint64_t fr_plan_pixels(const fr_plan *plan);   /* sum of w*h over the jobs */
/* how the plan's jobs are split between the render kernels (the decision is per job): the fast kernels — cov4_kernel
 * (4 x 4 or 2 x 2 samples) / win1_kernel (one sample per pixel) — take cells of ANY width and height up to 2048 sample
 * rows (renderGlyph's own image sizes, render_glyph.zig:14-19, included: strips of 64 / 128 / 256 pixels chosen from
 * the job's width, stores clipped at the cell's border) of glyphs with <= 768 segments; the general render_kernel takes
 * everything else                                                                                              */
int fr_plan_stats(const fr_plan *plan, uint32_t *n_jobs_cov4, uint32_t *n_jobs_general);
/* the kernel instances one render of the plan launches, as rocprofv3 --kernel-trace names them, each with its job
 * count: "fr::cov4_kernel<4, 32, 4, 4> x20992; fr::render_kernel<3, 4, 32, -1> x3" (NUL-terminated, truncated to cap);
 * a FR_FILL_CONSISTENT plan's instances carry a trailing 1: "fr::cov4_kernel<4, 32, 4, 4, 1> x20992"                  */
int fr_plan_describe(const fr_plan *plan, char *buf, size_t cap);

/* ---- text runs (BUILD-DEFINED) ---------------------------------------------------------------
 * The reference draws a line of text: each glyph at a pen position in font units, the pen advanced by the glyph's
 * advance_width (Appli.zig:318-349), every instance into one MSAA framebuffer, a sample lit if ANY instance covers it.
 * A text plan renders sets of such instances ("runs"), each into one finished image.
 *   Placement {glyph, pen_x64, pen_y}: pen_x64 is the image x of the glyph's font-unit origin in 1/64 pixel (26.6 fixed
 *     point); pen_y is the baseline's image row (whole rows; fr_glyph_place_ex, below, keeps the baseline to 1/64 pixel).  Image coordinates are the
 *     run's own: (0, 0) is its top-left pixel.
 *   Run {first, count, w, h, out_x, out_y, scale}: placements places[first .. first+count); it owns the whole w x h
 *     rectangle at (out_x, out_y) of the output and writes every pixel of it (0 where no glyph reaches).  Runs must not
 *     overlap each other.
 *   Instance cell: ix = floor(pen_x64 / 64), fx = (pen_x64 mod 64) / 64; renderGlyph's grid of the glyph at the run's
 *     scale (min_x = floor(x_min*scale), max_x = ceil(x_max*scale), min_y, max_y likewise, binary32 as fr_atlas_layout)
 *     gives a cell of (max_x - min_x + 1 + (fx != 0)) x (max_y - min_y + 1) pixels whose column 0 sits at image column
 *     ix + min_x and whose row 0 at image row pen_y - max_y; the cell is clipped to the run.
 *   Sample (i, j) of image pixel (X, Y) inside the cell:
 *       cx = (f32(X - ix) + (off(i) - fx)) / scale,   cy = (f32(pen_y - Y) - off(j)) / scale,   off(k) = (k + phase)/n
 *     (off(i) - fx is exact: both are multiples of 1/64 in (-1, 1)).  So an instance is an ordinary fr_job whose column
 *     offsets are shifted by fx, and with fx = 0 it is that job.  Outside its cell an instance contributes nothing.
 *   Value: the union over instances of the non-zero test.  FR_COVERAGE_U8 (n in {1, 2, 4}): round_half_up(255 k / n^2),
 *     k = # of sub-samples at which SOME instance has winding != 0; FR_MASK_NONZERO (n = 1): 255 if any instance's
 *     winding != 0.  Both phases; FR_FILL_CONSISTENT applies per instance.  FR_WINDING_I16, FR_GRAY_DEBUG and FR_SDF_U8
 *     have no meaning for overlapping instances: FR_E_UNSUPPORTED.                                                      */
typedef struct fr_glyph_place {
    uint32_t glyph;            /* index into the glyph set                                      */
    int32_t  pen_x64;          /* image x of the glyph's font-unit origin, 1/64 pixel            */
    int32_t  pen_y;            /* image row of the baseline                                      */
} fr_glyph_place;

typedef struct fr_text_run {
    uint32_t first, count;     /* places[first .. first + count)                                 */
    uint32_t w, h;             /* the run's image, pixels: every one of them is written          */
    uint32_t out_x, out_y;     /* its (0, 0) in the output, elements / rows                      */
    float    scale;            /* font_size / units_per_em                                       */
} fr_text_run;

/* An ordinary fr_plan (fr_plan_render / _render_timed / _describe / _stats / _pixels / _destroy and the "graph" /
 * "overlap" options all apply; fr_plan_pixels is the sum of the runs' w*h, fr_plan_stats counts every instance as
 * general: text_kernel evaluates the records of any glyph directly).  FR_E_INVALID: overlapping runs, a placement
 * range or glyph index out of range, unknown flag bits; FR_E_UNSUPPORTED: a mode / n outside the definition above;
 * the scale and coordinate limits of fr_plan_create apply to every run and instance cell.                          */
int fr_text_plan_create(fr_ctx *ctx, const fr_glyphset *gs, const fr_glyph_place *places, uint32_t n_places,
                        const fr_text_run *runs, uint32_t n_runs, const fr_raster_params *params, uint32_t flags,
                        fr_plan **out);

/* ---- RGBA text runs (BUILD-DEFINED) ------------------------------------------------------------
 * The reference's visible product: text in a colour (shaders/shader.slang: (225, 105, 180), alpha 1) blended into an
 * RGBA MSAA framebuffer cleared to (0, 0, 0, 0) (VulkanContext.zig:59, :188-192), glyphs drawn in order, the samples
 * averaged by the resolve.  An RGBA text plan has the placements, runs, cells, clipping, sample points and per-instance
 * non-zero test of a text plan (above), and colours: placement k has C_k = place_rgba[4k .. 4k+4) = (R, G, B, A), run r
 * the clear colour Q_r = run_clear_rgba[4r .. 4r+4).
 *   Every sub-sample s of every pixel of run r starts at Q_r.  The run's instances are applied in placement order: an
 *   instance k whose cell holds the pixel and whose winding at s is non-zero updates the sample by the reference's blend
 *   state (colour src*srcAlpha + dst*(1 - srcAlpha); alpha factors ONE, ZERO: VulkanContext.zig:1296-1305) in integers,
 *       c' = (C_k.c * A + c * (255 - A) + 127) div 255    for c in R, G, B    (round to nearest; no ties occur)
 *       a' = A                                                               (alpha replaced)
 *   Resolve: each channel of the pixel is (sum over the n x n sub-samples of v_s + n^2/2) div n^2, n in {1, 2, 4}
 *   (n = 1 is the reference's MSAA off).
 * So: clear (0,0,0,0) with every instance (255,255,255,255) gives every channel equal to the text plan's FR_COVERAGE_U8
 * byte; with A = 255 the last covering instance wins per sample; an instance with A = 0 keeps RGB and sets alpha to 0;
 * the order of overlapping placements matters.
 * The output element is 4 bytes, R G B A in memory, NOT premultiplied: the framebuffer's bytes.  With a (0,0,0,0) clear
 * colour and opaque text, RGB comes out premultiplied by the coverage, as in the reference's transparent window.
 * (FR_TEXT_OVER, below, updates alpha by source-over instead of replacing it: the element is then premultiplied.)
 * Without FR_TEXT_SRGB, blending is on the stored 8-bit values, as on a UNORM framebuffer.
 * params->mode must be FR_COVERAGE_U8 with n in {1, 2, 4}, either phase (another mode or n: FR_E_UNSUPPORTED; an unknown
 * mode value stays FR_E_INVALID, as for fr_text_plan_create); FR_FILL_CONSISTENT
 * applies per instance.  A NULL colour array with a non-zero count is FR_E_INVALID; every other check of
 * fr_text_plan_create applies.  The result is an ordinary fr_plan; out_dev must be 4-byte aligned (FR_E_INVALID), and
 * out_stride / out_x / out_rows and the 2^26 pitch limit count RGBA pixels.  fr_plan_pixels stays a pixel count;
 * fr_plan_describe names text_rgba_kernel<n, fill, blend> (blend = 0 when every placement colour has A = 255), or
 * text_srgb_kernel<n, fill, blend> for an FR_TEXT_SRGB plan.
 *
 * Flags of fr_text_plan_create_rgba only (every other entry point that takes flags keeps returning FR_E_INVALID for
 * them); both combine with each other and with FR_FILL_CONSISTENT.  Bit 2 is not assigned: it stays FR_E_INVALID everywhere,
as it was for fr_text_plan_create_rgba before these flags existed:
 *   FR_TEXT_SRGB  blend and resolve in linear light, as the reference's B8G8R8A8_SRGB / SRGB_NONLINEAR swapchain
 *       (VulkanContext.zig:834) does: the stored bytes are sRGB, decoded before blending and encoded after it, per sample.
 *       With f the IEC 61966-2-1 decode (c <= 0.04045 ? c / 12.92 : ((c + 0.055) / 1.055)^2.4) in binary64:
 *           D[v] = floor(65535 f(v / 255) + 1/2)                v in 0 .. 255   (fr_srgb_decode: 16-bit linear light)
 *           E(L) = #{k in 1 .. 255 : L >= T[k]},  T[k] = ceil(65535 f((k - 1/2) / 255))   (fr_srgb_encode: round to
 *                  nearest in the encoded domain, L in 0 .. 65535)
 *       A sample starts at Q_r; an instance k with C_k = (R, G, B, A) whose winding at it is non-zero updates it by
 *           c' = E((D[C_k.c] * A + D[c] * (255 - A) + 127) div 255)    for c in R, G, B
 *           a' = A                                                    (alpha is stored linearly, the blend unchanged)
 *       Resolve: each colour channel is E((sum over the n x n sub-samples of D[v_s] + n^2/2) div n^2); alpha as above.
 *       So: with n = 1 and every A = 255 the output equals the plan without FR_TEXT_SRGB byte for byte; the alpha channel
 *       always equals it; A = 0 keeps RGB; with A = 255 the last covering instance wins per sample; white (255,255,255,
 *       255) over (0,0,0,0) gives RGB = E(round(65535 k / n^2)) for the k of n^2 samples the text plan lights (50 % of
 *       white over black: 188, not 128).  Vulkan leaves the precision of blending to the implementation, so this integer
 *       form is the definition here, not a claim of bit parity with any driver.
 *   FR_TEXT_BGRA  the output element is B G R A in memory instead of R G B A (the swapchain's order); the colour arrays
 *       stay R G B A.  Equivalent to swapping R and B in every placement and clear colour, with or without FR_TEXT_SRGB.
 */
#define FR_TEXT_BGRA 4u
#define FR_TEXT_SRGB 8u

/* FR_TEXT_LOAD  (fr_text_plan_create_rgba only) draw over the pixels already in the output, as Vulkan's
 *       VK_ATTACHMENT_LOAD_OP_LOAD does: the same as drawing the existing image into the MSAA target as an opaque
 *       full-screen quad before the glyphs.
 *   Start value: every sub-sample of a pixel P of run r starts at the value P holds in the output when the render
 *       reaches it in stream order; Q_r is not used.  With FR_TEXT_SRGB the stored bytes are sRGB, decoded by D above;
 *       with FR_TEXT_BGRA the stored element is read as B G R A, as it is written.  The per-sample non-zero test, the
 *       blend in placement order (alpha replaced by A), the resolve, the cells and the clipping are unchanged.
 *   Consequences:
 *     1. A pixel at which no instance lights any sample comes back byte-identical: (n^2 v + n^2/2) div n^2 = v, and for
 *        sRGB E(D[v]) = v for all 256 values (true of the tables above).
 *     2. If the output holds Q_r in every pixel of run r, the result equals the same plan without FR_TEXT_LOAD and with
 *        clear colour Q_r, byte for byte.
 *     3. A render is not idempotent: rendering twice composites over the first result, which starts from resolved pixels.
 *   run_clear_rgba may be NULL and is ignored.  Runs still must not overlap; a pixel outside every run is neither read
 *   nor written.  Within a run the unit is the 64 x 16 tile (from the run's top-left pixel): only the tiles some clipped
 *   instance cell meets are launched, and a pixel of any other tile is neither read nor written, so text on a large
 *   image costs the tiles under the text.  In a launched tile every pixel of the run is read, and may be written back
 *   (unchanged, by consequence 1, where no sample is lit).  A plan whose instances are all clipped away launches
 *   nothing, but fr_plan_render still checks the output as for the same plan with a visible glyph.  Combines with FR_TEXT_SRGB,
 *   FR_TEXT_BGRA and FR_FILL_CONSISTENT; every other entry point that takes flags returns FR_E_INVALID for it.
 *   fr_plan_describe names text_rgba_load_kernel<n, fill, blend> (text_srgb_load_kernel<n, fill, blend> with
 *   FR_TEXT_SRGB) with the instance count; fr_plan_pixels stays the sum of the runs' w*h.                              */
#define FR_TEXT_LOAD 32u

int fr_text_plan_create_rgba(fr_ctx *ctx, const fr_glyphset *gs, const fr_glyph_place *places, const uint8_t *place_rgba,
                             uint32_t n_places, const fr_text_run *runs, const uint8_t *run_clear_rgba, uint32_t n_runs,
                             const fr_raster_params *params, uint32_t flags, fr_plan **out);

/* ---- text placements with their own size, slant and sub-pixel baseline (BUILD-DEFINED) ---------
 * fr_text_plan_create / fr_text_plan_create_rgba with a wider placement: the reference shows text under a view
 * transform with a float offset in both axes (Appli.zig zoom / drag; shader.slang: position * transform.scale +
 * transform.offset), so a line's baseline is not on a pixel row in general.  Runs, modes, n, phases, flags
 * (FR_FILL_CONSISTENT; for the RGBA form FR_TEXT_SRGB, FR_TEXT_BGRA, FR_TEXT_LOAD), colours, blending, resolve, clipping
 * to the run, "every pixel of the run is written" and the error codes are those of the two entry points above.  Only
 * the instance geometry differs.  All arithmetic below is binary32, one rounding per written operation, no fused
 * multiply-add.
 *   For a placement let s = scale != 0 ? scale : run.scale, k = slant, ix = floor(pen_x64 / 64), fx = (pen_x64 mod 64)
 *   / 64, iy = floor(pen_y64 / 64), fy = (pen_y64 mod 64) / 64 (floor and non-negative mod), and the glyph's box
 *   (x_min, y_min, x_max, y_max) as floats.
 *   Cell: lo = min(x_min + k*y_min, x_min + k*y_max), hi = max(x_max + k*y_min, x_max + k*y_max);
 *     min_x = floor(lo * s), max_x = ceil(hi * s), min_y = floor(y_min * s), max_y = ceil(y_max * s).  The cell is
 *     (max_x - min_x + 1 + (fx != 0)) columns by (max_y - min_y + 1 + (fy != 0)) rows; its column 0 is image column
 *     ix + min_x, its row 0 image row iy - max_y.  It is clipped to the run.  Outside its cell an instance contributes
 *     nothing (the cell is part of the definition: the reference's winding is not zero everywhere outside an outline).
 *   Sample (i, j) of image pixel (X, Y) inside the cell, off(q) = (q + phase) / n:
 *       cy = (f32(iy - Y) + (fy - off(j))) / s
 *       t  = (f32(X - ix) + (off(i) - fx)) / s
 *       cx = t - k * cy
 *     (fy - off(j) and off(i) - fx are exact: multiples of 1/64 in (-1, 1)).  The winding at (cx, cy) is the reference's
 *     (or FR_FILL_CONSISTENT's) for the glyph's own integer points, per instance: a point (x, y) of the outline is drawn
 *     at (x + k*y, y), the outlines themselves are not sheared.
 *   Validation: scale is 0 or finite, positive and inside the limits of a run's scale (2^-20 .. 2^20: FR_E_UNSUPPORTED
 *     outside; NaN, infinite or negative: FR_E_INVALID); slant is finite (else FR_E_INVALID) and |slant| <= 4 (76
 *     degrees; FR_E_UNSUPPORTED beyond); the pen and cell limits of fr_text_plan_create apply to iy and the sheared cell.
 *   So: (1) with pen_y64 = 64 * pen_y, scale 0 (or the run's) and slant 0, cell and samples are those of fr_glyph_place
 *   bit for bit; (2) adding 64 to every pen_y64 of a run moves its image down by exactly one row.
 * fr_plan_describe names text_place_kernel<n, fill>, or text_place_rgba_kernel / text_place_srgb_kernel /
 * text_place_rgba_load_kernel / text_place_srgb_load_kernel<n, fill, blend>, with the instance count.  Rotation is
 * fr_glyph_place_affine, below: it makes the ray height differ per lane and has its own kernels.                       */
typedef struct fr_glyph_place_ex {
    uint32_t glyph;     /* index into the glyph set                                                  */
    int32_t  pen_x64;   /* image x of the glyph's font-unit origin, 1/64 pixel (as fr_glyph_place)   */
    int32_t  pen_y64;   /* image y of the baseline, 1/64 pixel, downwards: 64 * pen_y is row pen_y   */
    float    scale;     /* this placement's font_size / units_per_em; 0: the run's scale             */
    float    slant;     /* k: a point (x, y) of the outline is drawn at (x + k*y, y); 0: upright     */
} fr_glyph_place_ex;

int fr_text_plan_create_ex(fr_ctx *ctx, const fr_glyphset *gs, const fr_glyph_place_ex *places, uint32_t n_places,
                           const fr_text_run *runs, uint32_t n_runs, const fr_raster_params *params, uint32_t flags,
                           fr_plan **out);
int fr_text_plan_create_rgba_ex(fr_ctx *ctx, const fr_glyphset *gs, const fr_glyph_place_ex *places,
                                const uint8_t *place_rgba, uint32_t n_places, const fr_text_run *runs,
                                const uint8_t *run_clear_rgba, uint32_t n_runs, const fr_raster_params *params,
                                uint32_t flags, fr_plan **out);

/* FR_TEXT_CACHE  (fr_text_plan_create, fr_text_plan_create_rgba, fr_text_plan_create_ex, fr_text_plan_create_rgba_ex)
 *       rasterise each distinct glyph image of the plan once per render and let every placement that shows it read it,
 *       as a text stack's glyph cache does.  The plan renders, byte for byte, what the same plan without the flag renders:
 *       every mode, n, phase, flag combination, clipping case, the LOAD tile rule and "every pixel of the run is written".
 *       Only the work differs.
 *   Key: the placements that survive clipping are grouped by (glyph, pen_x64 mod 64, bits of the run's scale) for
 *       fr_glyph_place, and by (glyph, pen_x64 mod 64, pen_y64 mod 64, bits of the effective scale, bits of the slant)
 *       for fr_glyph_place_ex; floats compare as bit patterns (0.0 and -0.0 are two keys).  By the sample definitions
 *       above, two placements of one key have identical n^2-bit sample masks at equal offsets from (ix, iy).
 *   Mask cell: each key owns the placement's whole, unclipped cell (cw x ch as defined above) as cw * ch elements of
 *       uint16_t, row-major with pitch cw: element (c, r) is the non-zero mask (bit j*n + i: sample (i, j)) of the pixel
 *       at cell column c, row r.  The cells live in one plan-owned store on the device.
 *   Render: "every render starts from the glyph points" stays: the prepare kernel as before, then one launch that fills
 *       every mask cell from the records, then one composite launch over the plan's tiles, in stream order on the
 *       context's stream; the composite is the cover / colour computation of the plan without the flag, with an
 *       instance's mask loaded from its key's cell at (X - c0, Y - r0), (c0, r0) = (ix + min_x, iy - max_y) the unclipped
 *       cell's origin.  The "graph" option captures the three launches.
 *   Cost: the flag buys nothing when no two placements share a key (every glyph image is then still made once, and
 *       stored and loaded besides), and it always costs the mask store: 2 bytes per element of every cell, allocated at
 *       plan creation.  It pays when many placements share few keys: running text on whole-pixel pens, or a fixed set of
 *       sub-pixel positions.
 *   Limits: the cells of one plan may hold at most 2^31 elements in all: FR_E_UNSUPPORTED beyond, decided on the host
 *       before anything is allocated; a device allocation failure is FR_E_NOMEM.  A plan whose placements are all clipped
 *       away has no cell and is the plan without the flag.
 *   Combines with FR_FILL_CONSISTENT and, on the RGBA entry points, with FR_TEXT_SRGB, FR_TEXT_BGRA, FR_TEXT_LOAD and
 *   FR_TEXT_OVER.  The
 *   two _affine entry points and every other entry point that takes flags return FR_E_INVALID for it.  Bits 2, 16, 64 and
 *   1 << 31 stay unassigned.
 *   fr_plan_describe lists the prepare kernel with the glyph count, glyph_mask_kernel<n, fill> with the cell count, and
 *   the composite with the instance count: text_cached_kernel<n>, or text_cached_rgba_kernel / text_cached_srgb_kernel /
 *   text_cached_rgba_load_kernel / text_cached_srgb_load_kernel<n, blend> (the fill rule acts only where masks are made, and
 *   one composite serves both placement forms).  fr_plan_pixels and fr_plan_stats are unchanged.                        */
#define FR_TEXT_CACHE 128u

/* FR_TEXT_OVER  (the RGBA text entry points: fr_text_plan_create_rgba, _rgba_ex, _rgba_affine) source-over alpha:
 *       the alpha half of Porter-Duff "over" on a premultiplied target, Vulkan's alpha factors ONE, ONE_MINUS_SRC_ALPHA
 *       in place of the reference's ONE, ZERO.
 *   Everything of an RGBA text plan is unchanged except the alpha a covered sample receives: the start value (Q_r, or the
 *       stored pixel under FR_TEXT_LOAD), the per-instance non-zero test, the placement order, the update of R, G and B
 *       (UNORM and FR_TEXT_SRGB forms), the resolve, the cells, the clipping and the LOAD tile rule.  An instance with
 *       C_k = (R, G, B, A) whose winding at the sample is non-zero updates the sample's alpha by
 *           a' = (255 * A + a * (255 - A) + 127) div 255
 *       the colour formula with C = 255 and the same exact rounding; alpha is stored linearly with or without
 *       FR_TEXT_SRGB.  C * A + c * (255 - A) is premultiplied source-over when the destination is premultiplied, so the
 *       output is read and written as PREMULTIPLIED R G B A (under FR_TEXT_SRGB: premultiplied in linear light);
 *       fr_rgba_unpremultiply turns a finished layer into straight alpha.
 *   Consequences:
 *     1. R, G and B of every pixel equal those of the same plan without the flag, byte for byte; only alpha can differ.
 *     2. If every placement colour has A = 255 the plan is the plan without the flag, byte for byte, and launches the
 *        same kernel instance (blend = 0).
 *     3. An instance with A = 0 leaves a sample entirely unchanged (without the flag it sets alpha to 0).
 *     4. Under FR_TEXT_LOAD over pixels whose alpha is 255, every alpha stays 255.
 *     5. Over a (0,0,0,0) clear, one instance (R, G, B, A) that covers k of the n^2 samples of a pixel gives alpha
 *        (k * A + n^2/2) div n^2.
 *   Combines with FR_FILL_CONSISTENT, FR_TEXT_SRGB, FR_TEXT_BGRA, FR_TEXT_LOAD and, where that flag is accepted,
 *   FR_TEXT_CACHE; every other entry point that takes flags returns FR_E_INVALID for it.  Bits 2, 16, 64 and 1 << 31 stay
 *   unassigned.  fr_plan_describe names the plan's kernel with blend = 2 (..._kernel<n, fill, 2>, text_cached_..._kernel<n,
 *   2>) when the flag is set and some placement colour has A != 255.                                                    */
#define FR_TEXT_OVER 256u

/* ---- text placements with a 2 x 2 matrix: rotated, mirrored and sheared text (BUILD-DEFINED) ----
 * fr_text_plan_create_ex / fr_text_plan_create_rgba_ex with a matrix per placement: vertical axis titles, text along a
 * direction, a rotated view, mirrored text.  Runs, modes, n in {1, 2, 4}, both phases, the flags (FR_FILL_CONSISTENT; for
 * the RGBA form FR_TEXT_SRGB, FR_TEXT_BGRA, FR_TEXT_LOAD), colours, blend order, resolve, clipping to the run, "every
 * pixel of the run is written", the LOAD tile rule and the error codes are those of the _ex entry points.
 * fr_text_run::scale is validated as before but not used by these placements.  Only the instance geometry differs.  All
 * arithmetic below is binary32 with one rounding per written operation and no fused multiply-add, except the inverse
 * matrix, which is binary64.
 *   For a placement let (xx, xy, yx, yy) = m: the font-unit point (x, y), y up, is drawn xx*x + xy*y pixels right of and
 *   yx*x + yy*y pixels above the pen.  ix, fx, iy, fy come from pen_x64 and pen_y64 exactly as for fr_glyph_place_ex.
 *   Inverse (host, once per placement, binary64 from the four floats): D = xx*yy - xy*yx as two rounded products and one
 *     rounded difference, no fused multiply-add; q00 = f32(yy / D), q01 = f32(-xy / D), q10 = f32(-yx / D),
 *     q11 = f32(xx / D).
 *   Cell: for the four corners (x, y) of the glyph's box as floats, u = f32(xx*x) + f32(xy*y), v = f32(yx*x) + f32(yy*y);
 *     min_x = floor(min u), max_x = ceil(max u), min_y = floor(min v), max_y = ceil(max v).  The cell is
 *     (max_x - min_x + 1 + (fx != 0)) columns by (max_y - min_y + 1 + (fy != 0)) rows; its column 0 is image column
 *     ix + min_x, its row 0 image row iy - max_y.  It is clipped to the run.  Outside its cell an instance contributes
 *     nothing; inside it every sample counts: there is no further gate in glyph space.  Without FR_FILL_CONSISTENT the
 *     reference's false windings on sample rows through vertices are therefore reproduced wherever the cell reaches, and
 *     under a rotation such a row is a slanted line across the cell, not an image row: FR_FILL_CONSISTENT is recommended
 *     for rotated text.
 *   Sample (i, j) of image pixel (X, Y) inside the cell, off(q) = (q + phase) / n:
 *       dx = f32(X - ix) + (off(i) - fx)            dy = f32(iy - Y) + (fy - off(j))
 *       cx = f32(q00 * dx) + f32(q01 * dy)          cy = f32(q10 * dx) + f32(q11 * dy)
 *     The winding at (cx, cy) is the reference's (or FR_FILL_CONSISTENT's) for the glyph's own integer points, per
 *     instance.  A negative D (mirrored text) is valid: the non-zero test does not depend on orientation.
 *   Validation: any m not finite, or D == 0: FR_E_INVALID.  Any |m| > 2^20 or any |q| > 2^20: FR_E_UNSUPPORTED.  The pen
 *     and cell limits of fr_text_plan_create apply to iy and the cell above.
 *   So: (1) with m = {s, s*k, 0, s} and s a power of two, the cell and every sample are bit for bit those of
 *   fr_glyph_place_ex with scale s and slant k (multiplying by the exact 1/s and by -k/s rounds as the division and the
 *   product do); (2) adding 64 to every pen_y64 of a run moves its image down by exactly one row, and adding 64 to every
 *   pen_x64 moves it right by exactly one column; (3) m = {0, -s, s, 0} is a quarter turn counter-clockwise.
 * fr_plan_describe names text_affine_kernel<n, fill>, or text_affine_rgba_kernel / text_affine_srgb_kernel /
 * text_affine_rgba_load_kernel / text_affine_srgb_load_kernel<n, fill, blend>, with the instance count.  Every lane
 * solves every record at its own ray height, so these plans cost more than the upright forms, most at a quarter turn
 * (DESIGN.md section 4.7).  Perspective and one matrix per run are not offered.                 */
typedef struct fr_glyph_place_affine {
    uint32_t glyph;     /* index into the glyph set                                                       */
    int32_t  pen_x64;   /* image x of the glyph's font-unit origin, 1/64 pixel                            */
    int32_t  pen_y64;   /* image y of it, 1/64 pixel, downwards (as fr_glyph_place_ex)                    */
    float    m[4];      /* xx, xy, yx, yy: the font-unit point (x, y), y up, is drawn                     */
                        /* xx*x + xy*y pixels right of and yx*x + yy*y pixels above the pen               */
} fr_glyph_place_affine;

int fr_text_plan_create_affine(fr_ctx *ctx, const fr_glyphset *gs, const fr_glyph_place_affine *places, uint32_t n_places,
                               const fr_text_run *runs, uint32_t n_runs, const fr_raster_params *params, uint32_t flags,
                               fr_plan **out);
int fr_text_plan_create_rgba_affine(fr_ctx *ctx, const fr_glyphset *gs, const fr_glyph_place_affine *places,
                                    const uint8_t *place_rgba, uint32_t n_places, const fr_text_run *runs,
                                    const uint8_t *run_clear_rgba, uint32_t n_runs, const fr_raster_params *params,
                                    uint32_t flags, fr_plan **out);

/* FR_TEXT_CACHE_AFFINE  (fr_text_plan_create_affine, fr_text_plan_create_rgba_affine) FR_TEXT_CACHE for the matrix form:
 *       rasterise each distinct glyph image of the plan once per render and let every placement that shows it read it.
 *       The plan renders, byte for byte, what the same plan without the flag renders: every mode, n in {1, 2, 4}, both
 *       phases, FR_FILL_CONSISTENT, FR_TEXT_SRGB, FR_TEXT_BGRA, FR_TEXT_LOAD, FR_TEXT_OVER, every clipping case, the LOAD
 *       tile rule and "every pixel of the run is written".  Only the work differs.
 *   Key: the placements that survive clipping are grouped by (glyph, pen_x64 mod 64, pen_y64 mod 64, the bit patterns of
 *       m[0], m[1], m[2], m[3]); floats compare as bit patterns (0.0 and -0.0 are two keys).  The key holds the caller's
 *       matrix, not its inverse: the cell is defined from m, and equal m gives equal q.  By the sample definition above,
 *       two placements of one key have identical n^2-bit sample masks at equal offsets from (ix, iy).
 *   Mask cell: each key owns the placement's whole, unclipped cell (cw x ch as the matrix form defines it: the four mapped
 *       corners, + 1, + (fx != 0), + (fy != 0)) as cw * ch elements of uint16_t, row-major with pitch cw: element (c, r)
 *       is the non-zero mask (bit j*n + i: sample (i, j)) of the pixel at cell column c, row r.  The cells live in one
 *       plan-owned store on the device.
 *   Render: the prepare kernel as before, then one launch that fills every mask cell from the records, then the composite
 *       launch of FR_TEXT_CACHE plans (it does not depend on the placement form), in stream order on the context's
 *       stream.  The "graph" option captures the three launches.
 *   Cost: as for FR_TEXT_CACHE.  A cell is the bounding box of the mapped glyph box, so at 45 degrees it holds about twice
 *       the area the glyph does; the flag pays where many placements share few (glyph, pen fraction, matrix) keys:
 *       running text under one matrix on a fixed set of sub-pixel pens, or the 3x-wide plane of sub-pixel (LCD) text.
 *   Limits: those of FR_TEXT_CACHE: at most 2^31 elements over all cells of a plan (FR_E_UNSUPPORTED beyond, decided on the
 *       host before anything is allocated); a device allocation failure is FR_E_NOMEM.  A plan whose placements are all
 *       clipped away has no cell and is the plan without the flag.
 *   Combines with FR_FILL_CONSISTENT and, on the RGBA entry point, with FR_TEXT_SRGB, FR_TEXT_BGRA, FR_TEXT_LOAD and
 *   FR_TEXT_OVER.  The upright, _ex and raster entry points and every other entry point that takes flags return
 *   FR_E_INVALID for it; FR_TEXT_CACHE stays FR_E_INVALID on the two _affine entry points, so the two bits together are
 *   refused everywhere.  Bits 2, 16, 64 and 1 << 31 stay unassigned.
 *   fr_plan_describe lists the prepare kernel with the glyph count, glyph_mask_affine_kernel<n, fill> with the cell count
 *   and the composite of FR_TEXT_CACHE plans with the instance count.  fr_plan_pixels and fr_plan_stats are unchanged.   */
#define FR_TEXT_CACHE_AFFINE 512u

/* One-shot: plan + render + copy back.  out_host: HOST buffer (caller-allocated,
 * e.g. Image.Gray.data / Image.Winding.data from the Zig allocator).  Synchronous.  */
int fr_render_batch(fr_ctx *ctx, const fr_glyphset *gs, const fr_job *jobs, uint32_t n_jobs,
                    const fr_raster_params *params, void *out_host, size_t out_stride, size_t out_rows);
int fr_render_batch_ex(fr_ctx *ctx, const fr_glyphset *gs, const fr_job *jobs, uint32_t n_jobs,
                       const fr_raster_params *params, uint32_t flags, void *out_host, size_t out_stride, size_t out_rows);

/* ---- renderGlyph drop-in (render_glyph.zig:11-33) -------------------------
 * fr_render_glyph_dims reproduces :13-19 on the host so the caller can size the
 * Image.Gray first; fr_render_glyph fills it: w*h u8, row-major, value per `mode`
 * (FR_GRAY_DEBUG is what the reference's renderGlyph returns).                      */
int fr_render_glyph_dims(const int16_t box[4], uint16_t units_per_em, uint16_t font_size,
                         int16_t min_corner[2], int16_t max_corner[2],
                         uint16_t *width, uint16_t *height, float *scale);
int fr_render_glyph(fr_ctx *ctx, const int16_t *points_xy, const uint32_t *contour_start,
                    uint32_t n_contours, const int16_t box[4], uint16_t units_per_em,
                    uint16_t font_size, int32_t mode, void *out_host);
int fr_render_glyph_ex(fr_ctx *ctx, const int16_t *points_xy, const uint32_t *contour_start,
                       uint32_t n_contours, const int16_t box[4], uint16_t units_per_em,
                       uint16_t font_size, int32_t mode, uint32_t flags, void *out_host);

/* ---- exact-integer path (render_glyph.zig:76-300) -------------------------
 * fr_glyph_info_init: GlyphInfo.init (:110-146) — one CurveType (:84-95 enum order)
 * and one include_p0 flag per curve, contours back to back, computed on the device.
 * fr_winding_in_glyph: windingInGlyph (:160-247) at n_query integer font-unit points.
 * fr_winding_lattice: the lattice Image.GlyphDebug.render walks (Image.zig:227-236):
 * (x_max-x_min+3) x (y_max-y_min+3) int16, point (x_min+w-1, y_max-h+1).
 * Predicates use 128-bit integers: identical to the reference's i64 wherever that
 * does not overflow.                                                  */
int fr_glyph_info_init(fr_ctx *ctx, const int16_t *points_xy, const uint32_t *contour_start,
                       uint32_t n_contours, uint8_t *curve_type, uint8_t *include_p0);
int fr_winding_in_glyph(fr_ctx *ctx, const int16_t *points_xy, const uint32_t *contour_start,
                        uint32_t n_contours, const int16_t *query_xy, uint32_t n_query,
                        int16_t *out_winding);
int fr_winding_lattice(fr_ctx *ctx, const int16_t *points_xy, const uint32_t *contour_start,
                       uint32_t n_contours, const int16_t box[4], int16_t *out_host);

/* Image.GlyphDebug.render (Image.zig:220-240): the lattice of fr_winding_lattice coloured by
 * setWindingLinear (:192-200; overflow colour 150) with the glyph's on-curve / control points marked
 * {255,255,0} / {0,255,255} by setGlyphPoints (:202-218, in the reference's order).  rgb_host receives
 * (x_max-x_min+3) * (y_max-y_min+3) RGB triples, row-major — Image.RGB.data (Image.zig:132-170).        */
int fr_glyph_debug_render(fr_ctx *ctx, const int16_t *points_xy, const uint32_t *contour_start,
                          uint32_t n_contours, const int16_t box[4], uint8_t winding_scale, uint8_t *rgb_host);

/* ---- exact-integer sampling on a K-times refined lattice (BUILD-DEFINED) ----
 * GlyphInfo.init + windingInGlyph (render_glyph.zig:110-146, :160-300) applied, rule for rule, to
 * the glyph whose points are multiplied by K (1 <= K <= 8, so the 128-bit predicates cannot
 * overflow), at the integer points (x0 + i, y0 - j), i < w, j < h of that scaled glyph — i.e. at
 * the font-unit points ((x0+i)/K, (y0-j)/K) with no floating point anywhere.  K = 1 is the
 * reference's own lattice.  fr_exact_coverage evaluates n x n lattice points per pixel
 * (lattice (w_px*n) x (h_px*n)) and writes round_half_up(255 * #{winding != 0} / n^2), the same
 * box-filtered non-zero fill as FR_COVERAGE_U8 on the integer inside test.  The reference has no
 * such mode (its exact path is dead code used only by GlyphDebug at K = 1); parity is against the
 * oracle's twin of the same definition.                                                        */
int fr_exact_lattice(fr_ctx *ctx, const int16_t *points_xy, const uint32_t *contour_start,
                     uint32_t n_contours, uint32_t K, int32_t x0, int32_t y0, uint32_t w, uint32_t h,
                     int16_t *out_host /* [h][w] */);
int fr_exact_coverage(fr_ctx *ctx, const int16_t *points_xy, const uint32_t *contour_start,
                      uint32_t n_contours, uint32_t K, int32_t x0, int32_t y0, uint32_t w_px, uint32_t h_px,
                      uint32_t n, uint8_t *out_host /* [h_px][w_px] */);

/* ---- atlas layout (host side; BUILD-DEFINED: the reference has no atlas) -------------------
 * The fixed cell grid every atlas of this library uses: glyph i of `n_glyphs` (index first_glyph + i in
 * the glyph set, box boxes[4 i ..]) gets a cell x cell window whose pixel (0,0) is the glyph's own
 * renderGlyph origin — scale = f32(font_size) / f32(units_per_em), min_x = floor(x_min * scale),
 * max_y = ceil(y_max * scale) in binary32 exactly as render_glyph.zig:13-17 — at column (i % cols),
 * row (i / cols) of a cols-wide grid.  rows_per_page > 0 cuts the grid into pages of that many cell rows
 * (a 2048^2 page of 128-pixel cells: cols = rows_per_page = 16): out_y restarts on every page and
 * page_of_job[i] (if not NULL) names the page; *n_pages (if not NULL) receives the page count.
 * units_per_em: n_upm = 1 (one font) or n_upm = n_glyphs (one value per glyph).                      */
int fr_atlas_layout(const int16_t *boxes, uint32_t n_glyphs, uint32_t first_glyph,
                    const uint16_t *units_per_em, uint32_t n_upm, uint16_t font_size,
                    uint32_t cell, uint32_t cols, uint32_t rows_per_page,
                    fr_job *jobs_out, uint32_t *page_of_job, uint32_t *n_pages);

/* The reference's own product shape in batch: glyph i gets exactly the image renderGlyph would allocate for it —
 * fr_render_glyph_dims' W x H, pixel (0,0) at (min_x, max_y) (render_glyph.zig:13-19, :26-27) — shelf-packed in input
 * order into an atlas `atlas_w` elements wide: left to right, out_x rounded up to a multiple of `align` (1: tight),
 * a new shelf when the next image does not fit; *atlas_h (if not NULL) receives the rows used.  Every job's bytes are
 * what fr_render_glyph writes for that glyph (tests).                                                          */
int fr_atlas_layout_glyph_dims(const int16_t *boxes, uint32_t n_glyphs, uint32_t first_glyph,
                               const uint16_t *units_per_em, uint32_t n_upm, uint16_t font_size,
                               uint32_t atlas_w, uint32_t align, fr_job *jobs_out, uint32_t *atlas_h);

/* ---- multi-GPU assembly (optional; SURVEY section 8e: "optional final assembly: all-gather of row bands") --------
 * The hot path needs no collective: every rank renders its own glyph range into its own band.  When one rank (or all)
 * wants the whole atlas, the bands are equal-sized slices of one buffer — rank r rendered into
 * atlas_dev + r * band_bytes — and this call runs RCCL's in-place ncclAllGather over them on the context's stream.
 * nccl_comm is an ncclComm_t the HOST created (ncclCommInitRank / torch.distributed own the rendezvous; the library
 * never does); the call binds to the RCCL that is already loaded in the process (dlsym, no link-time dependency) and
 * returns FR_E_UNSUPPORTED if there is none.  Asynchronous like fr_plan_render: fr_ctx_sync / stream order apply.   */
int fr_allgather_bands(fr_ctx *ctx, void *nccl_comm, void *atlas_dev, size_t band_bytes);
/* The same assembly onto ONE rank: rank `root` receives every other rank's band into that rank's slot of ITS atlas_dev
 * (one RCCL group of ncclRecv's), every other rank sends its own band (atlas_dev + rank * band_bytes) and receives
 * nothing — each peer's bytes cross its own xGMI link to the root once, instead of every rank ingesting the whole atlas.
 * root < 0 is fr_allgather_bands.  Asynchronous on the context's stream.                                              */
int fr_gather_bands(fr_ctx *ctx, void *nccl_comm, void *atlas_dev, size_t band_bytes, int root);

/* ---- contour producer (host side): TrueType glyf/loca -> Glyph contour layout ------------
 * What font/Font.zig + font/ttf.zig + font/Glyph.zig do in the reference (Font.initTTF :31,
 * loadGlyph :171, SimpleGlyph.initFromReader ttf.zig:759, ComponentGlyph ttf.zig:830,
 * Contour.initTTF Glyph.zig:43, initTTFComponent :108, transform1 :178), restated in C++ so
 * whole fonts can be batch-fed to fr_glyphset_create without the Zig host.  The font bytes are
 * copied; glyphs are parsed lazily and cached like Font.glyphs.  Where the reference
 * @panic("not impl")s these return FR_E_UNSUPPORTED (hinted glyphs unless FR_FONT_ALLOW_HINTED).
 * fr_font_glyph_measure gives the sizes to allocate, fr_font_glyph_fill writes the i16 (x,y)
 * points and the n_contours+1 contour offsets (relative to the glyph, starting at 0).           */
typedef struct fr_font fr_font;
#define FR_FONT_ALLOW_HINTED 1u
int fr_font_open(const void *ttf_bytes, size_t len, uint32_t flags, fr_font **out);
void fr_font_close(fr_font *font);
int fr_font_info(const fr_font *font, uint16_t *units_per_em, uint16_t *num_glyphs, int *y0_baseline);
int fr_font_char_to_glyph(const fr_font *font, uint32_t codepoint, uint16_t *glyph_index);
/* Font.getGlyph's advance_width (Font.zig:161-169, hmtx read as Font.zig:123-139 reads it), font units */
int fr_font_glyph_advance(const fr_font *font, uint16_t glyph_index, int16_t *advance_width);
int fr_font_glyph_measure(fr_font *font, uint16_t glyph_index, uint32_t *n_contours, uint32_t *n_points, int16_t box[4]);
int fr_font_glyph_fill(fr_font *font, uint16_t glyph_index, int16_t *points_xy, uint32_t *contour_start);

/* The reference's pen walk (Appli.zig:318-349; host only): glyph_index_out[k] = cmap(codepoints[k]) (0 if unmapped),
 * E_k = sum_{m<k} advance_width(m) in font units (the i16 of fr_font_glyph_advance), and
 *     pen_x64_out[k] = floor((128 * font_size * E_k + upm) / (2 * upm))     (exact int64: E_k * font_size / upm in 1/64
 * pixel, rounded half up); *end_pen_x64 (if not NULL) the same for E_n.  No kerning and no line breaking: the reference
 * has neither.                                                                                                         */
int fr_text_layout(const fr_font *font, const uint32_t *codepoints, uint32_t n, uint16_t font_size,
                   uint16_t *glyph_index_out, int32_t *pen_x64_out, int32_t *end_pen_x64);

/* Where a line's decorations belong (host only; BUILD-DEFINED: the reference reads none of these tables).  All values are
 * in font units, y up, as the font stores them: hhea's ascender, descender and lineGap; post's underlinePosition (the TOP of
 * the underline) and underlineThickness; OS/2's yStrikeoutSize and yStrikeoutPosition (the top of the stroke).  A font
 * without a post or OS/2 table, or with one too short to hold these fields, opens as before: its bit of `present` is clear
 * and its values are 0.                                                                                                  */
typedef struct fr_font_line {
    int16_t ascender, descender, line_gap;              /* hhea */
    int16_t underline_position, underline_thickness;    /* post; 0 when absent */
    int16_t strikeout_size, strikeout_position;         /* OS/2; 0 when absent */
    uint16_t present;                                   /* bit 0: post, bit 1: OS/2 */
} fr_font_line;
int fr_font_line_metrics(const fr_font *font, fr_font_line *out);

/* The rows of a decoration at font_size, as offsets from the baseline in 1/64 pixel, y DOWN (add them to a placement's
 * pen_y64), rounded as fr_text_layout rounds a pen: R(v) = floor((128 * font_size * v + upm) / (2 * upm)), exact, with a
 * true floor for negative v.
 *     FR_DECOR_UNDERLINE:  top = -R(underline_position),  bottom = top + max(1, R(underline_thickness))
 *     FR_DECOR_STRIKEOUT:  top = -R(strikeout_position),  bottom = top + max(1, R(strikeout_size))
 *     FR_DECOR_LINE_BOX:   top = -R(ascender),            bottom = -R(descender)
 * [top, bottom) x the line's pen span, as an fr_layer_rect, is the underline, the stroke or the box a highlight fills.
 * FR_E_UNSUPPORTED when the table the kind needs is absent; FR_E_INVALID for an unknown kind or a NULL argument.          */
#define FR_DECOR_UNDERLINE 0u
#define FR_DECOR_STRIKEOUT 1u
#define FR_DECOR_LINE_BOX  2u
int fr_text_decoration(const fr_font *font, uint16_t font_size, uint32_t kind, int32_t *top_y64, int32_t *bottom_y64);

/* ---- QOI writer (host side), byte-compatible with tools/qoi.zig:25-88 saveRGB -----------
 * RGB-only stream, op order RUN -> INDEX -> DIFF -> LUMA -> RGB, run cap 62, BE header, 8-byte
 * trailer.  fr_qoi_encode_gray feeds an Image.Gray (or an atlas page) through getRGBLinear =
 * {v,v,v} (Image.zig:78-82).  *n_out receives the stream length; FR_E_INVALID if cap is short. */
size_t fr_qoi_bound(uint32_t width, uint32_t height);
int fr_qoi_encode_rgb(const uint8_t *rgb, uint32_t width, uint32_t height, uint8_t *out, size_t cap, size_t *n_out);
int fr_qoi_encode_gray(const uint8_t *gray, uint32_t width, uint32_t height, size_t stride, uint8_t *out, size_t cap, size_t *n_out);
/* A standard 4-channel QOI stream (the QOI specification, not tools/qoi.zig, which writes RGB only): channels tag 4,
 * QOI_OP_RGBA when alpha changes, the index hash r*3 + g*5 + b*7 + a*11, previous pixel (0,0,0,255) before the first.
 * rgba: 4 bytes per pixel, rows stride_px pixels apart (>= width).  Worst case 22 + 5 * width * height bytes.          */
int fr_qoi_encode_rgba(const uint8_t *rgba, uint32_t width, uint32_t height, size_t stride_px, uint8_t *out, size_t cap, size_t *n_out);

/* ---- sRGB conversions (host side) of FR_TEXT_SRGB plans: D and E as defined at fr_text_plan_create_rgba -------------
 * fr_srgb_decode: out[i] = D[in[i]] (16-bit linear light); fr_srgb_encode: out[i] = E(in[i]).  n values each; NULL with
 * n > 0 is FR_E_INVALID.                                                                                               */
int fr_srgb_decode(const uint8_t *in, size_t n, uint16_t *out);
int fr_srgb_encode(const uint16_t *in, size_t n, uint8_t *out);

/* ---- premultiplied -> straight alpha (host side), for the output of FR_TEXT_OVER plans ---------------------------------
 * In place, n_pixels elements of 4 bytes with alpha last (R G B A or B G R A alike).  Per pixel with alpha a:
 *     a = 0:                   (0, 0, 0, 0)
 *     otherwise, srgb = 0:     c = min(255, (255 * c + a div 2) div a)                       for the three colour bytes
 *     otherwise, srgb != 0:    c = E(min(65535, (255 * D[c] + a div 2) div a))               (D, E: FR_TEXT_SRGB above)
 * A pixel with a = 255 is unchanged in both spaces (E(D[v]) = v).  This is what the RGBA QOI writer and other
 * straight-alpha file formats expect.  NULL with n_pixels > 0 is FR_E_INVALID.                                          */
int fr_rgba_unpremultiply(uint8_t *rgba, size_t n_pixels, int srgb);

/* ---- compositing a finished layer (BUILD-DEFINED; DESIGN.md sections 4.8 and 5) ----------------------------------------
 * An RGBA text plan with FR_TEXT_OVER over a (0, 0, 0, 0) clear colour renders a premultiplied layer.  fr_layer_over puts
 * rectangles of such a layer over a premultiplied image on the device, at whole-pixel offsets and with an opacity: a
 * viewer that drags or fades text renders the layer once and composites it per frame.
 *   Both images are 4-byte elements with alpha last (R G B A or B G R A alike, provided the two agree), both
 *   PREMULTIPLIED (with FR_LAYER_SRGB: in linear light, as FR_TEXT_SRGB | FR_TEXT_OVER plans write them).  src_dev: the
 *   layer, src_rows rows of src_stride_px pixels; dst_dev: the image, dst_rows rows of dst_stride_px pixels.  An image's
 *   width, for clipping, is its stride.
 *   Definition: m(x, y) = (x * y + 127) div 255 (round to nearest; 255 is odd, so no ties occur).  For a layer pixel
 *   (s_c, s_a), the destination pixel (d_c, d_a) under it, c over the three colour bytes, and the blit's opacity o:
 *       a'    = m(s_a, o)
 *       out_a = a' + m(d_a, 255 - a')                                  (both colour spaces; never exceeds 255)
 *       out_c = min(255, m(s_c, o) + m(d_c, 255 - a'))                 (flags = 0: on the stored values, UNORM)
 *       out_c = E(min(65535, (D[s_c] * o + 127) div 255 + (D[d_c] * (255 - a') + 127) div 255))       (FR_LAYER_SRGB; D and
 *                                                                       E as defined at fr_text_plan_create_rgba)
 *   Consequences:
 *     1. A layer pixel (0, 0, 0, 0), or o = 0, leaves the destination pixel byte-identical in both spaces (m(x, 255) = x,
 *        m(x, 0) = 0, E(D[v]) = v).
 *     2. A layer pixel with s_a = 255 under o = 255 replaces the destination pixel.
 *     3. A destination alpha of 255 stays 255.
 *     4. A valid premultiplied UNORM layer pixel (s_c <= s_a) never reaches the clamp.
 *     5. The layer of a plan with FR_TEXT_OVER, n = 1 and every placement alpha 255, rendered over the clear colour
 *        (0, 0, 0, 0) and composited with o = 255 at (0, 0) onto a frame, equals the same plan rendered with FR_TEXT_LOAD
 *        onto that frame, byte for byte, with and without FR_TEXT_SRGB (FR_LAYER_SRGB to match).  For translucent colours
 *        or n > 1 the two routes round in two steps against one and differ in the last bit here and there: no equality is
 *        promised.
 *   Geometry: blit k copies the w x h rectangle at (src_x, src_y) of the layer so that its top-left pixel lands on
 *     (dst_x, dst_y) of the image.  The rectangle must lie inside the layer (src_x + w <= src_stride_px, src_y + h <=
 *     src_rows: FR_E_INVALID otherwise); its destination is clipped to [0, dst_stride_px) x [0, dst_rows), and a blit that
 *     is clipped away entirely is valid.  After clipping, the destination rectangles of one call must not overlap each
 *     other, and the byte ranges of the two images must not overlap (FR_E_INVALID).  Inside a clipped rectangle any pixel
 *     may be read, and written back unchanged; outside every clipped rectangle no byte of the image is read or written; no
 *     byte of the layer is ever written.
 *   Validation: both pointers non-NULL and 4-byte aligned, both strides within the 2^26-element pitch limit of
 *     fr_plan_render, blits non-NULL when n_blits > 0, every opacity <= 255, no unknown flag bit (FR_E_INVALID each);
 *     n_blits = 0 is valid and launches nothing.  FR_E_UNSUPPORTED: an image of 2^31 rows or more, or a call whose clipped
 *     rectangles need more than 2^22 tiles of 256 x 16 pixels.
 *   Execution: one launch of layer_over_kernel<srgb, opacity> (opacity = 0 when every blit that draws has o = 255) for
 *     all blits of the call, behind a small kernel that brings the call's tile table into device memory; asynchronous on
 *     the context's stream, in stream order after earlier renders as fr_plan_render is; the caller may reuse `blits` as
 *     soon as the call returns.
 * FR_LAYER_SRGB is the flag space of fr_layer_over, fr_layer_shadow, fr_layer_outline, fr_layer_rects, fr_layer_paint,
 * fr_layer_lcd, fr_layer_mask, fr_layer_warp and fr_layer_blend: no other entry point knows it, and these know none of the FR_TEXT_ / FR_FILL_ flags.  (FR_LCD_BGR = 2 is
 * fr_layer_lcd's alone: the others refuse it as an unknown bit.)                                                              */
#define FR_LAYER_SRGB 1u

typedef struct fr_layer_blit {
    uint32_t src_x, src_y;     /* top-left of the rectangle in the layer, pixels                 */
    uint32_t w, h;             /* its size; 0 x anything is valid and does nothing               */
    int32_t  dst_x, dst_y;     /* where that top-left lands in the destination; may be negative  */
    uint32_t opacity;          /* o in 0 .. 255 (above: FR_E_INVALID); 255 = the layer as it is  */
} fr_layer_blit;

int fr_layer_over(fr_ctx *ctx, const void *src_dev, size_t src_stride_px, size_t src_rows,
                  void *dst_dev, size_t dst_stride_px, size_t dst_rows,
                  const fr_layer_blit *blits, uint32_t n_blits, uint32_t flags);

/* fr_rgba_unpremultiply on the device: the same three cases, in place, over the w x h window at rgba_dev of an image with
 * rows of stride_px pixels; byte for byte what the host function makes of the same pixels, and no byte outside the window
 * is read or written.  Asynchronous on the context's stream.  FR_E_INVALID: NULL or a pointer that is not 4-byte aligned,
 * w > stride_px, stride_px beyond 2^26.                                                                                   */
int fr_layer_unpremultiply(fr_ctx *ctx, void *rgba_dev, size_t stride_px, uint32_t w, uint32_t h, int srgb);

/* ---- the shadow of a finished layer (BUILD-DEFINED; DESIGN.md sections 4.9 and 5) ----------------------------------------
 * fr_layer_shadow makes a drop shadow, a glow or an outline of a layer: the layer's alpha, spread by a square maximum,
 * blurred by up to three box passes, moved by whole pixels and tinted with one colour.  The result is itself a
 * premultiplied layer (R G B A, alpha last), so the caller composites it with fr_layer_over, then the text over it.
 *   All arithmetic is in integers; m, D and E are as defined above.
 *   Source alpha: A0(u, v) is the alpha byte of layer pixel (src_x + u, src_y + v) for 0 <= u < w, 0 <= v < h, and 0
 *     everywhere else on the integer plane.  No layer byte outside the window is read, and only alpha is read.
 *   Spread: A1(u, v) = max of A0(u + i, v + j) over |i| <= s, |j| <= s.
 *   Blur: with W = (2 r + 1)^2, for k = 1 .. p:
 *       A_{k+1}(u, v) = (sum of A_k(u + i, v + j) over |i| <= r, |j| <= r  +  W div 2) div W
 *     Each two-dimensional pass rounds once to 8 bits; the sum is exact, so any evaluation order gives the same bytes.
 *     r = 0 or p = 0 skips the stage.
 *   Tint: for pixel (X, Y) of the destination rectangle, 0 <= X < dst_w, 0 <= Y < dst_h:
 *       alpha = A_last(X - dx, Y - dy),  a = m(alpha, rgba[3])
 *       stored = (m(R, a), m(G, a), m(B, a), a)                                              (flags = 0)
 *       stored = (E((D[R] * a + 127) div 255), E((D[G] * a + 127) div 255), E((D[B] * a + 127) div 255), a)   (FR_LAYER_SRGB)
 *     The sRGB form is what an FR_TEXT_SRGB | FR_TEXT_OVER plan writes for one fully covered sample of colour (C, a) over
 *     a (0, 0, 0, 0) clear.  Byte order is R G B A; a caller with B G R A layers swaps rgba[0] and rgba[2].
 *   Writes: every pixel of the destination rectangle is written and none of it is read.  No byte of the destination
 *     outside the rectangle is read or written.  No layer byte is written.
 *   Consequences:
 *     1. With s = 0, no blur, dx = dy = 0 and colour (255, 255, 255, 255) the output is (alpha, alpha, alpha, alpha) of the
 *        layer.
 *     2. A stage leaves a constant neighbourhood unchanged: (v W + W div 2) div W = v.  Text-interior alpha 255 stays 255.
 *     3. alpha is non-zero only within Chebyshev distance R = s + p r of a window pixel with non-zero alpha.  A rectangle
 *        padded by R holds the whole shadow; a rectangle out of reach is all (0, 0, 0, 0).
 *     4. Adding 1 to dx or dy moves the image by exactly one column or row.
 *     5. The definition is symmetric in the axes: a transposed window with dx and dy swapped gives the transposed image.
 *     6. One pixel of alpha 255 with p = 1 gives (255 + W div 2) div W on exactly the (2 r + 1)^2 square around it.
 *   Validation, in this order.  FR_E_INVALID: NULL ctx; an unknown flag bit; a NULL or not 4-byte aligned image pointer,
 *     or a stride beyond 2^26 (the layer, then the destination).  FR_E_UNSUPPORTED: an image of 2^31 rows or more.
 *     FR_E_INVALID: NULL `shadow`; a window of non-zero area that is not inside the layer (src_x + w <= src_stride_px,
 *     src_y + h <= src_rows); a rectangle of non-zero area that is not inside dst_stride_px x dst_rows; s > 8, r > 32 or
 *     p > 3; overlapping byte ranges of the two images.  FR_E_UNSUPPORTED: a rectangle of more than 2^22 tiles of 64 x 64
 *     pixels, counted as ceil((dst_w + 3) / 64) * ceil(dst_h / 64) (fr_layer_over's limit of 2^34 pixels); a call whose two
 *     intermediate planes (one byte per pixel each) would exceed 2^30 bytes together.
 *     w, h, dst_w or dst_h of 0 is valid: dst_w = 0 or dst_h = 0 writes nothing, a window of zero area writes zeros over
 *     the rectangle.  Any int32 dx or dy is valid.
 *   Execution: one kernel per stage (the last one fused with the tint; a single kernel when there is no stage),
 *     asynchronous on the context's stream, in stream order with renders and composites.  The intermediate planes belong
 *     to the context and grow on demand; growing waits for the stream.  The caller may reuse `shadow` as soon as the call
 *     returns.
 * The parameters' type is fr_layer_shadow_params: C keeps typedef names and functions in one name space.                  */
typedef struct fr_layer_shadow_params {
    uint32_t src_x, src_y, w, h;          /* the window of the layer whose alpha casts the shadow      */
    uint32_t dst_x, dst_y, dst_w, dst_h;  /* the rectangle of the destination that receives it         */
    int32_t  dx, dy;                      /* destination pixel (X, Y) of the rectangle shows window
                                             coordinate (X - dx, Y - dy)                               */
    uint32_t spread;                      /* s in 0 .. 8                                               */
    uint32_t blur_radius;                 /* r in 0 .. 32                                              */
    uint32_t blur_passes;                 /* p in 0 .. 3; r = 0 or p = 0 means no blur                 */
    uint8_t  rgba[4];                     /* the shadow's colour, straight R G B A                     */
} fr_layer_shadow_params;

int fr_layer_shadow(fr_ctx *ctx, const void *src_dev, size_t src_stride_px, size_t src_rows,
                    void *dst_dev, size_t dst_stride_px, size_t dst_rows,
                    const fr_layer_shadow_params *shadow, uint32_t flags);   /* 0 or FR_LAYER_SRGB */

/* ---- round outlines of a finished layer (BUILD-DEFINED; DESIGN.md sections 4.13 and 5) -----------------------------------
 * fr_layer_outline grows or shrinks the shape of a layer by a disc of radius rho / 16 pixels, anti-aliased, and tints the
 * result: an outline to composite under the text (GROW), the outline alone for hollow or translucent text (RING), a line
 * inside the edge to draw over the text (INNER), or the shrunk shape (SHRINK).  The result is itself a premultiplied layer
 * (R G B A, alpha last), as fr_layer_shadow's is.  A spread of fr_layer_shadow is a maximum over a square, so its outlines
 * have square corners and whole-pixel widths; this maximum is weighted by a disc.
 *   All arithmetic is in integers; m, D and E are as defined above.
 *   Source alpha: A0(u, v) is exactly fr_layer_shadow's: the alpha byte of layer pixel (src_x + u, src_y + v) for
 *     0 <= u < w, 0 <= v < h, and 0 everywhere else on the integer plane.  No layer byte outside the window is read, and
 *     only alpha is read.
 *   Disc weight, for an integer offset (i, j), with rho = radius:
 *       q = isqrt(65536 (i^2 + j^2))                      (the floor of 256 times the distance)
 *       t = 16 rho + 256 - q
 *       K(i, j) = 0 if t <= 0, else min(255, (255 t + 128) div 256)
 *     a linear ramp one pixel wide that ends at distance rho / 16 + 1.  K(0, 0) = 255 for every rho, and K is 0 beyond
 *     Chebyshev distance R = ceil(rho / 16).
 *   Grow:   G[A](u, v) = max of m(A(u + i, v + j), K(i, j)) over |i| <= R, |j| <= R.
 *   Shrink: S(u, v) = 255 - G[255 - A0](u, v); the complement 255 - A0 is 255 outside the window.
 *   Alpha by kind:
 *       FR_OUTLINE_GROW    G[A0]
 *       FR_OUTLINE_RING    G[A0] - A0        (never negative: K(0, 0) = 255 and m(a, 255) = a)
 *       FR_OUTLINE_INNER   A0 - S
 *       FR_OUTLINE_SHRINK  S
 *   Tint and writes: fr_layer_shadow's, word for word.  For pixel (X, Y) of the destination rectangle, 0 <= X < dst_w,
 *     0 <= Y < dst_h: alpha is the kind's alpha at (X - dx, Y - dy), a = m(alpha, rgba[3]), and
 *       stored = (m(R, a), m(G, a), m(B, a), a)                                              (flags = 0)
 *       stored = (E((D[R] * a + 127) div 255), E((D[G] * a + 127) div 255), E((D[B] * a + 127) div 255), a)   (FR_LAYER_SRGB)
 *     Every pixel of the destination rectangle is written and none of it is read.  No byte of the destination outside the
 *     rectangle is read or written.  No layer byte is written.
 *   Consequences:
 *     1. rho = 0, GROW: the bytes of fr_layer_shadow with no stage and the same colour, in both colour spaces.  RING and
 *        INNER give zeros, SHRINK equals GROW.
 *     2. One pixel of alpha 255, GROW, colour (255, 255, 255, 255): the alpha plane is the table K around it.
 *     3. rho = 16 k: a vertical or horizontal edge moves by exactly k pixels: columns 255 .. 255, 128, 0 .. become the same
 *        row shifted by k.  rho = 8 puts K(1, 0) = 128 on the first pixel beyond a hard edge.
 *     4. shadow(no stage) <= GROW <= shadow(spread = R, no blur) pointwise in alpha.  GROW is non-zero only within Chebyshev
 *        distance R of a window pixel with non-zero alpha; INNER and SHRINK are zero outside the window.
 *     5. Adding 1 to dx or dy moves the image by exactly one column or row.
 *     6. The definition has the square's eight symmetries: a transposed or mirrored window gives the transposed or mirrored
 *        image.
 *     7. GROW does not decrease and SHRINK does not increase as rho grows.
 *     The maximum of the raw products A * K followed by one (x + 127) div 255 equals the maximum of the m's (m is monotone),
 *     which is how the kernel evaluates it.
 *   Validation, in this order.  FR_E_INVALID: NULL ctx; an unknown flag bit; a NULL or not 4-byte aligned image pointer,
 *     or a stride beyond 2^26 (the layer, then the destination).  FR_E_UNSUPPORTED: an image of 2^31 rows or more.
 *     FR_E_INVALID: NULL `outline`; a window of non-zero area that is not inside the layer; a rectangle of non-zero area
 *     that is not inside dst_stride_px x dst_rows; radius > FR_OUTLINE_MAX_RADIUS or kind > FR_OUTLINE_SHRINK; overlapping
 *     byte ranges of the two images.  FR_E_UNSUPPORTED: a rectangle of more than 2^22 tiles of 64 x 64 pixels, counted as
 *     ceil((dst_w + 3) / 64) * ceil(dst_h / 64).  w, h, dst_w or dst_h of 0 is valid: dst_w = 0 or dst_h = 0 writes nothing,
 *     a window of zero area writes zeros over the rectangle for every kind.  Any int32 dx or dy is valid.
 *   Execution: one launch of layer_outline_kernel behind the small kernel that brings the call's weight table into device
 *     memory, with no intermediate plane; asynchronous on the context's stream, in stream order with renders, composites
 *     and shadows.  A rectangle that the outline cannot reach takes fr_layer_shadow's zero-writing launch.  The caller may
 *     reuse `outline` as soon as the call returns.                                                                          */
#define FR_OUTLINE_GROW   0u   /* the layer's shape grown by the radius: composite it under the text      */
#define FR_OUTLINE_RING   1u   /* grown minus the layer: the outline alone (hollow or translucent text)    */
#define FR_OUTLINE_INNER  2u   /* the layer minus its shrunk shape: a line inside the edge, drawn over it   */
#define FR_OUTLINE_SHRINK 3u   /* the layer's shape shrunk by the radius                                    */
#define FR_OUTLINE_MAX_RADIUS 256u

typedef struct fr_layer_outline_params {
    uint32_t src_x, src_y, w, h;          /* the window of the layer, as fr_layer_shadow_params        */
    uint32_t dst_x, dst_y, dst_w, dst_h;  /* the rectangle of the destination that receives it         */
    int32_t  dx, dy;                      /* destination pixel (X, Y) of the rectangle shows window
                                             coordinate (X - dx, Y - dy)                               */
    uint32_t radius;                      /* rho, in 1/16 pixel, 0 .. 256 (16 pixels)                  */
    uint32_t kind;                        /* FR_OUTLINE_*                                              */
    uint8_t  rgba[4];                     /* the outline's colour, straight R G B A                    */
} fr_layer_outline_params;

int fr_layer_outline(fr_ctx *ctx, const void *src_dev, size_t src_stride_px, size_t src_rows,
                     void *dst_dev, size_t dst_stride_px, size_t dst_rows,
                     const fr_layer_outline_params *outline, uint32_t flags);   /* 0 or FR_LAYER_SRGB */

/* ---- anti-aliased rectangles over an image (BUILD-DEFINED; DESIGN.md sections 4.10 and 5) ----------------------------------
 * fr_layer_rects fills axis-aligned rectangles with sub-pixel edges, each in one straight colour, over a premultiplied
 * image on the device: underlines, strike-outs, selections behind text, carets, panels.  fr_text_decoration gives the rows
 * of the first three.
 *   The destination is what fr_layer_over's is: dst_rows rows of dst_stride_px elements of 4 bytes, alpha last,
 *   PREMULTIPLIED (with FR_LAYER_SRGB: in linear light); its width, for clipping, is its stride.  m, D and E as above.
 *   Coverage is the exact area of the rectangle inside the pixel.  For pixel column X and row Y:
 *       cx = max(0, min(x1, 64 (X + 1)) - max(x0, 64 X))         (0 .. 64; cy likewise from y0, y1 and Y)
 *       k  = (255 * cx * cy + 2048) div 4096                     (0 .. 255)
 *   Source: a = m(k, rgba[3]).  A pixel with a = 0 is left byte-identical.
 *   Composite, for colour byte C of the rectangle over the destination pixel (d_c, d_a):
 *       out_a = a + m(d_a, 255 - a)
 *       out_c = min(255, m(C, a) + m(d_c, 255 - a))                                                   (flags = 0)
 *       out_c = E(min(65535, (D[C] * a + 127) div 255 + (D[d_c] * (255 - a) + 127) div 255))          (FR_LAYER_SRGB)
 *     m(C, a) <= a, so the clamp is never reached on a valid premultiplied destination (d_c <= d_a).  Byte order is
 *     R G B A; a caller with B G R A images swaps rgba[0] and rgba[2].
 *   Order: rectangles MAY overlap (fr_layer_over's blits may not): rectangle j is composited over the result of rectangles
 *     0 .. j - 1, per pixel.
 *   Consequences:
 *     1. A pixel-aligned rectangle with rgba[3] = 255 replaces its pixels with (R, G, B, 255) in both spaces.
 *     2. With flags = 0 the result equals a route through the other two calls: a layer whose alpha plane is k(X, Y),
 *        tinted by fr_layer_shadow with no stage and colour rgba, composited by fr_layer_over at o = 255, byte for byte.
 *     3. That is not promised with FR_LAYER_SRGB: the shadow stores an encoded 8-bit colour and so rounds once more; this
 *        call blends the colour's 16-bit linear value directly.
 *     4. Moving all four edges of a rectangle by 64 moves its image by exactly one pixel.
 *     5. The definition is symmetric in the axes.
 *     6. Outside the outward-rounded, clipped bounding box of every rectangle no byte of the image is read or written;
 *        inside one, a pixel may be read and written back unchanged.
 *   Not promised: two rectangles that split a pixel between them do not add up to full coverage (coverages are
 *     composited, not summed); and a rectangle is not the bytes a text plan makes of a block glyph with the same edges
 *     (text counts samples, this is area).
 *   Validation, in this order.  FR_E_INVALID: NULL ctx; an unknown flag bit; a NULL or not 4-byte aligned dst_dev; a stride
 *     beyond 2^26.  FR_E_UNSUPPORTED: 2^31 rows or more.  FR_E_INVALID: NULL `rects` with n_rects > 0.  FR_E_UNSUPPORTED:
 *     rectangles that meet more than 2^22 tiles of 256 x 16 pixels (tiles on the image's grid, each counted once), then more
 *     than 2^24 (tile, rectangle) pairs.  FR_E_NOMEM: a host allocation failed.
 *     Every value of the four int32 edges is valid (the arithmetic is in int64), x1 <= x0 or y1 <= y0 included; edges of
 *     int32 in 1/64 pixel cannot reach columns or rows beyond 2^25, so wider images are only drawn into up to there.
 *     n_rects = 0 launches nothing; nor does a call whose rectangles are all empty, clipped away or fully transparent.
 *   Execution: one launch of layer_rects_kernel<srgb> for all rectangles of the call, one workgroup per tile that some
 *     rectangle meets, behind the small kernel that brings the call's tables into device memory; every pixel is loaded at
 *     most once and stored at most once however many rectangles cover it.  Asynchronous on the context's stream, in stream
 *     order with renders, composites and shadows; the caller may reuse `rects` as soon as the call returns.               */
typedef struct fr_layer_rect {
    int32_t x0, y0, x1, y1;   /* edges in 1/64 pixel of the destination, y down; x1 <= x0 or y1 <= y0: valid, draws nothing */
    uint8_t rgba[4];          /* straight R G B A */
} fr_layer_rect;

int fr_layer_rects(fr_ctx *ctx, void *dst_dev, size_t dst_stride_px, size_t dst_rows,
                   const fr_layer_rect *rects, uint32_t n_rects, uint32_t flags);   /* 0 or FR_LAYER_SRGB */

/* ---- linear and radial gradients through a layer's alpha (BUILD-DEFINED; DESIGN.md sections 4.11 and 5) --------------------
 * fr_layer_paint composites one gradient over a premultiplied image on the device, either through the alpha of a window
 * of a layer (gradient text; a gradient glow when the layer is a shadow) or, with src_dev = NULL, through full coverage
 * (a gradient panel).  Both images are what fr_layer_over's are; m, D and E as above.  All arithmetic is in integers.
 *   rdiv(n, d) = floor((2 n + d) / (2 d)) for d > 0 and n of either sign, in exact integers (floor throughout: a half-way
 *   case rounds up, also below zero).
 *   Coverage: destination pixel (X, Y) = (dst_x + u, dst_y + v), 0 <= u < w, 0 <= v < h, is drawn with cov = the alpha byte
 *     of layer pixel (src_x + u, src_y + v); with src_dev = NULL, cov = 255.  Only alpha is read from the layer, and
 *     nothing outside the window.  The rectangle is clipped to [0, dst_stride_px) x [0, dst_rows) as a blit of
 *     fr_layer_over is; a rectangle clipped away entirely is valid.
 *   Gradient parameter t, a signed 64-bit integer, 65536 to one gradient length, taken at the pixel's centre.  The four
 *     geometry values x0, y0, x1, y1 are in 1/64 pixel of the DESTINATION image, y down.
 *     FR_GRADIENT_LINEAR, from (x0, y0) to (x1, y1): dx = x1 - x0, dy = y1 - y0, L2 = dx^2 + dy^2,
 *         TX = rdiv(64 dx 2^32, L2),  TY = rdiv(64 dy 2^32, L2),  T0 = rdiv(((32 - x0) dx + (32 - y0) dy) 2^32, L2)
 *         t  = (T0 + X TX + Y TY) >> 16                            (arithmetic shift; the sum stays below 2^60)
 *       For X, Y < 32768, t differs from floor(65536 * the exact projection) by at most 1; it is exact where TX, TY and T0
 *       are (dyadic gradients).
 *     FR_GRADIENT_RADIAL, centre (x0, y0), radius r = x1 (y1 must be 0):
 *         ddx = 64 X + 32 - x0,  ddy = 64 Y + 32 - y0,  s = isqrt((ddx^2 + ddy^2) 256)        (the floor square root)
 *         R = rdiv(2^60, r),  t = floor(s R / 2^48)                                           (the full 128-bit product)
 *       |t - floor(65536 dist / r)| <= 1 + 4096 / r.
 *   Spread, t -> u in 0 .. 65535: FR_SPREAD_PAD: u = clamp(t, 0, 65535).  FR_SPREAD_REPEAT: u = t mod 65536 (floor mod).
 *     FR_SPREAD_REFLECT: v = t mod 131072, u = v < 65536 ? v : 131071 - v.
 *   Colour: a table G[0 .. 1023] of straight R G B A, built on the host.  Entry k is the gradient at q = 64 k + 32: stop 0
 *     if q < off[0]; stop n - 1 if q >= off[n - 1]; else with i the largest index with off[i] <= q (equal offsets make a
 *     hard edge, the later stop wins), wd = off[i + 1] - off[i], f = q - off[i], each of the four channels is
 *         (c_i (wd - f) + c_{i+1} f + wd div 2) div wd
 *     on the stored 8-bit straight values, in both colour spaces.  A pixel's colour is (R, G, B, A) = G[u >> 6].
 *   Composite: fr_layer_rects' with a = m(cov, A) and C the table colour; a = 0 leaves the pixel byte-identical.
 *   Consequences:
 *     1. One stop (R, G, B, A), src_dev = NULL: the bytes of fr_layer_rects with the pixel-aligned rectangle
 *        (64 dst_x, 64 dst_y, 64 (dst_x + w), 64 (dst_y + h)) of that colour, in both spaces.
 *     2. One stop and a layer, flags = 0: the bytes of fr_layer_shadow (no stage, that colour) of the window into a cleared
 *        layer, composited by fr_layer_over at o = 255.  Not promised with FR_LAYER_SRGB, for the reason given at
 *        fr_layer_rects' consequence 3.
 *     3. Over a (0, 0, 0, 0) destination the result is a valid premultiplied layer: the gradient-filled text, ready for
 *        fr_layer_over.
 *     4. Adding (64, 64) to the geometry's points (a radius stays) and (1, 1) to (dst_x, dst_y) moves the image by one
 *        pixel: exactly for a radial gradient and for a linear one whose TX, TY and T0 are exact; else t may move within
 *        its bound.
 *     5. A horizontal linear gradient (dy = 0) gives identical rows.  A radial one is symmetric about its centre when the
 *        centre is a pixel centre or a pixel corner.
 *     6. No destination byte is read or written outside the clipped rectangle (inside it a pixel may be read and written
 *        back unchanged); no layer byte is written; a pixel with cov = 0 or A = 0 is byte-identical.
 *   Validation, in this order.  FR_E_INVALID: NULL ctx; an unknown flag bit; a NULL or not 4-byte aligned dst_dev, or
 *     dst_stride_px beyond 2^26; with src_dev: not 4-byte aligned, or src_stride_px beyond 2^26; with src_dev = NULL: a
 *     non-zero src_stride_px or src_rows.  FR_E_UNSUPPORTED: an image of 2^31 rows or more.  FR_E_INVALID: NULL `paint`;
 *     with src_dev: a window of non-zero area that is not inside the layer; with src_dev = NULL: a non-zero src_x or
 *     src_y; an unknown kind or spread; n_stops outside 1 .. 8; an offset above 65536, or one below the offset before it;
 *     linear with L2 = 0; radial with r <= 0 or y1 != 0; overlapping byte ranges of the two images.  FR_E_UNSUPPORTED: a
 *     geometry value with |v| > 2^26; L2 < 4096 or r < 64 (a gradient shorter than one pixel); radial with |ddx| or
 *     |ddy| >= 2^27 at a corner pixel of the clipped rectangle; a clipped rectangle of more than 2^22 tiles of 256 x 16
 *     pixels.  w = 0 or h = 0 is valid and launches nothing.
 *   Execution: one launch of layer_paint_kernel<srgb, kind, layer or none>, one workgroup per 256 x 16 tile of the clipped
 *     rectangle, behind the small kernel that brings the call's colour table into device memory.  The destination is
 *     loaded only where some pixel of a lane's four has 0 < a < 255 and stored only where one has a != 0.  Asynchronous
 *     on the context's stream, in stream order with renders and the other layer calls; the caller may reuse `paint` as
 *     soon as the call returns.                                                                                            */
#define FR_GRADIENT_LINEAR 0u
#define FR_GRADIENT_RADIAL 1u
#define FR_SPREAD_PAD      0u
#define FR_SPREAD_REPEAT   1u
#define FR_SPREAD_REFLECT  2u
#define FR_GRADIENT_MAX_STOPS 8

typedef struct fr_gradient_stop {
    uint32_t offset;          /* 0 .. 65536, not below the stop before it */
    uint8_t  rgba[4];         /* straight R G B A */
} fr_gradient_stop;

typedef struct fr_layer_paint_params {
    uint32_t src_x, src_y;    /* top-left of the window in the layer, pixels (0 with src_dev = NULL)   */
    uint32_t w, h;            /* the rectangle's size; 0 x anything is valid and does nothing           */
    int32_t  dst_x, dst_y;    /* where that top-left lands in the destination; may be negative          */
    uint32_t kind;            /* FR_GRADIENT_LINEAR or FR_GRADIENT_RADIAL                               */
    uint32_t spread;          /* FR_SPREAD_PAD, _REPEAT or _REFLECT                                     */
    int32_t  x0, y0, x1, y1;  /* linear: from (x0, y0) to (x1, y1); radial: centre (x0, y0), radius x1,
                                 y1 = 0.  1/64 pixel of the destination, y down                         */
    uint32_t n_stops;         /* 1 .. FR_GRADIENT_MAX_STOPS                                             */
    fr_gradient_stop stops[FR_GRADIENT_MAX_STOPS];
} fr_layer_paint_params;

int fr_layer_paint(fr_ctx *ctx, const void *src_dev, size_t src_stride_px, size_t src_rows,
                   void *dst_dev, size_t dst_stride_px, size_t dst_rows,
                   const fr_layer_paint_params *paint, uint32_t flags);   /* 0 or FR_LAYER_SRGB */

/* ---- sub-pixel (LCD) text from a 3x-wide coverage plane (BUILD-DEFINED; DESIGN.md sections 4.12 and 5) ----------------------
 * fr_layer_lcd turns a coverage plane sampled at three times the horizontal resolution into per-channel anti-aliased
 * text over a premultiplied image on the device: a 5-tap FIR across sub-pixels, then a composite with an alpha of its own
 * for each of the three colour bytes.  The plane comes from the text plans as they are: fr_text_plan_create_affine with
 * m = {3 s, 0, 0, s}, the pens' x tripled and a run of 3 W x H gives a FR_COVERAGE_U8 plane whose element 3 u + j is
 * sub-pixel j of pixel u (12 sample columns per pixel at n = 4).  m, D and E as above.  All arithmetic is in integers.
 *   Plane: cov_rows rows of cov_stride bytes, one byte per element; any byte alignment of cov_dev and any cov_stride.  For
 *     a blit, c(q, v) is the byte at element src_x + q of row src_y + v for 0 <= q < 3 w and 0 <= v < h, and 0 everywhere
 *     else: bytes outside the window never influence the result.  Reads stay inside elements [0, cov_stride) of the rows
 *     src_y .. src_y + h - 1; no plane byte is written.
 *   Filter: W[0 .. 4] = weights, or (8, 77, 86, 77, 8) when weights is NULL; their sum must be exactly 256.  For window
 *     pixel (u, v) and sub-pixel j in 0 .. 2, with q = 3 u + j:
 *         f_j = (sum_i W[i] c(q + i - 2, v) + 128) div 256                                        (0 .. 255)
 *   Channel map: memory byte b in 0 .. 2 of the destination pixel takes f_b; with FR_LCD_BGR it takes f_{2-b} (in what
 *     follows f_b is the value byte b takes).  rgba[b] is always the colour of memory byte b: a caller with B G R A
 *     images swaps rgba[0] and rgba[2], as for the other calls.
 *   Composite: A = rgba[3], a_b = m(f_b, A); the destination pixel is (d_0, d_1, d_2, d_a).
 *     flags without FR_LAYER_SRGB:  out_b = min(255, m(rgba[b], a_b) + m(d_b, 255 - a_b))
 *     with FR_LAYER_SRGB:           out_b = E(min(65535, (D[rgba[b]] a_b + 127) div 255 + (D[d_b] (255 - a_b) + 127) div 255))
 *     alpha:                        a_max = max(a_0, a_1, a_2),  out_a = a_max + m(d_a, 255 - a_max)
 *   Geometry: window pixel (u, v) lands on destination pixel (dst_x + u, dst_y + v).  The window must lie inside the
 *     plane: src_x + 3 w <= cov_stride and src_y + h <= cov_rows.  The destination rectangle is clipped to [0,
 *     dst_stride_px) x [0, dst_rows) as a blit of fr_layer_over is; a blit clipped away entirely is valid.  Sub-pixels of
 *     clipped-away pixels still serve as taps.  After clipping, the rectangles of one call must not overlap, nor may the
 *     byte ranges of plane and image.  Outside the clipped rectangles no image byte is read or written; inside one, a
 *     pixel may be read and written back unchanged.
 *   Consequences:
 *     1. A pixel with a_0 = a_1 = a_2 = 0 is byte-identical, in both spaces.
 *     2. d_a = 255 stays 255.
 *     3. With flags = 0, the colour (255, 255, 255, 255) and a destination pixel (0, 0, 0, 255), the result is
 *        (f_0, f_1, f_2, 255).
 *     4. A constant run of plane value v filters to v: (256 v + 128) div 256 = v.
 *     5. With weights = (0, 0, 256, 0, 0) and a plane with c(3 u + j) = k(u) for all j, the bytes are those of
 *        fr_layer_paint with one stop of that colour through a layer whose alpha is k, in both spaces, with or without
 *        FR_LCD_BGR.
 *     6. With flags = 0 a valid premultiplied destination (d_b <= d_a) stays valid: g(a) = a + m(d_a, 255 - a) does not
 *        decrease with a, and m(C, a_b) <= a_b.
 *     7. Adding 3 to src_x moves the image by one pixel, adding 1 by one sub-pixel.
 *     8. FR_LCD_BGR equals swapping bytes 0 and 2 of the image and of the colour before and after the call without it.
 *     9. One element of 255 alone in a row gives f = (255 W[i] + 128) div 256 on five consecutive sub-pixels (W[4] on the
 *        first of them).
 *   Validation, in this order.  FR_E_INVALID: NULL ctx; an unknown flag bit; NULL cov_dev; cov_stride beyond 2^26; a NULL
 *     or not 4-byte aligned dst_dev; dst_stride_px beyond 2^26.  FR_E_UNSUPPORTED: 2^31 rows or more in either image.
 *     FR_E_INVALID: NULL blits with n_blits > 0; weights whose sum is not 256; a window of non-zero area that is not
 *     inside the plane; overlapping clipped rectangles; overlapping byte ranges of plane and image.  FR_E_UNSUPPORTED:
 *     more than 2^22 tiles of 256 x 16 pixels.  w = 0 or h = 0 is valid; n_blits = 0 launches nothing.
 *   Execution: one launch of layer_lcd_kernel<srgb> for all blits, one workgroup per 256 x 16 tile, behind the small kernel
 *     that brings the call's tile table into device memory.  The destination is loaded only where some pixel of a lane's
 *     four is touched (some a_b != 0) without all three a_b at 255, and stored only where one is touched.  Asynchronous on
 *     the context's stream, in stream order with renders and the other layer calls; the caller may reuse blits and weights
 *     as soon as the call returns.
 * FR_LCD_BGR lives in the flag space of the layer calls, beside FR_LAYER_SRGB, and only fr_layer_lcd knows it: fr_layer_over,
 * fr_layer_shadow, fr_layer_rects and fr_layer_paint refuse it as an unknown bit.                                             */
#define FR_LCD_BGR  2u
#define FR_LCD_TAPS 5

typedef struct fr_lcd_blit {
    uint32_t src_x, src_y;    /* plane element / row of sub-pixel 0 of window pixel (0, 0)              */
    uint32_t w, h;            /* size in DESTINATION pixels; the window is 3 w x h plane elements       */
    int32_t  dst_x, dst_y;    /* where window pixel (0, 0) lands; may be negative                       */
    uint8_t  rgba[4];         /* the text colour, straight R G B A                                      */
} fr_lcd_blit;

int fr_layer_lcd(fr_ctx *ctx, const void *cov_dev, size_t cov_stride, size_t cov_rows,
                 void *dst_dev, size_t dst_stride_px, size_t dst_rows,
                 const fr_lcd_blit *blits, uint32_t n_blits,
                 const uint16_t *weights /* FR_LCD_TAPS values, or NULL */, uint32_t flags);

/* ---- a layer through a mask, or an erase through one (BUILD-DEFINED; DESIGN.md sections 4.14 and 5) ------------------------
 * fr_layer_mask is fr_layer_over with an opacity per pixel: a second image, the mask, decides where the layer's pixels
 * land (text clipped to a rounded panel, a photo showing inside the glyphs, a soft wipe).  With FR_MASK_ERASE there is no
 * layer and the mask lowers the destination instead (destination-out: a knock-out, or underlines that skip the glyphs'
 * ink).  The layer and the destination are what fr_layer_over's are; m, D and E as defined there.  All integers.
 *   Mask value: for a pixel of the rectangle, k is the alpha byte of the mask pixel over it when the mask is a 4-byte
 *     layer (mask_stride in pixels, mask_dev 4-byte aligned); with FR_MASK_PLANE k is the byte of a plane of 1-byte
 *     elements, such as a coverage plan's output (mask_stride in bytes; any pointer and any pitch).  Then
 *         k' = invert ? 255 - k : k,      t = m(k', o)          (o: the blit's opacity)
 *   Composite (no FR_MASK_ERASE): fr_layer_over's definition with t in the place of o:
 *       a'    = m(s_a, t)
 *       out_a = a' + m(d_a, 255 - a')
 *       out_c = min(255, m(s_c, t) + m(d_c, 255 - a'))                                             (UNORM)
 *       out_c = E(min(65535, (D[s_c] * t + 127) div 255 + (D[d_c] * (255 - a') + 127) div 255))    (FR_LAYER_SRGB)
 *   Erase (FR_MASK_ERASE; src_dev must be NULL, src_stride_px and src_rows are ignored, and so are src_x and src_y):
 *       out_a = m(d_a, 255 - t)
 *       out_c = m(d_c, 255 - t)                                  (UNORM)
 *       out_c = E((D[d_c] * (255 - t) + 127) div 255)            (FR_LAYER_SRGB)
 *   Consequences:
 *     1. A mask that is 255 everywhere with invert = 0, or 0 everywhere with invert = 1, gives the bytes of fr_layer_over
 *        with the same rectangles and opacities, in both spaces (m(255, o) = o).
 *     2. Where t = 0 the destination pixel is byte-identical, in both spaces and both modes.
 *     3. A valid premultiplied layer pixel never reaches the clamp: m(s_c, t) <= m(s_a, t).
 *     4. A layer of one opaque colour (C0, C1, C2, 255) through a layer mask at opacity o gives the bytes of fr_layer_paint
 *        with the single stop (C0, C1, C2, A = o) through that mask layer's window, in both spaces: both reduce to
 *        a = m(k, o).
 *     5. FR_MASK_PLANE gives the bytes of the same call with a layer mask whose alpha bytes are the plane's.
 *     6. Erase: t = 255 stores (0, 0, 0, 0); a destination alpha never grows; the three colour bytes of an erase through an
 *        all-255 plane at opacity o equal those of fr_layer_rects with the pixel-aligned black rectangle of alpha o, in
 *        both spaces (the alpha differs: the rectangle's is o + m(d_a, 255 - o)).
 *     7. invert = 1 equals invert = 0 on the byte-complemented mask.
 *   Geometry: fr_layer_over's, with the mask added.  The rectangle must lie inside the layer (unless erasing) and inside
 *     the mask (mask_x + w <= mask_stride, mask_y + h <= mask_rows); its destination is clipped to the image; the clipped
 *     rectangles of one call must not overlap each other.  The destination's bytes must not overlap the layer's or the
 *     mask's; layer and mask may overlap each other or be the same memory (both are only read).  No byte of the layer or
 *     the mask is written, no byte outside the mask's mask_stride x mask_rows elements is read, and outside every
 *     clipped rectangle no byte of the image is read or written.
 *   Validation, in this order.  FR_E_INVALID: NULL ctx; an unknown flag bit (FR_LCD_BGR is one); a bad dst (NULL, not
 *     4-byte aligned, a pitch above 2^26); a bad mask (NULL, a pitch above 2^26 elements, a layer mask that is not 4-byte
 *     aligned); FR_MASK_ERASE with a non-NULL src_dev, or no FR_MASK_ERASE with a NULL one; a bad src.  FR_E_UNSUPPORTED:
 *     2^31 rows or more in any image.  FR_E_INVALID: NULL blits with n_blits > 0; the destination overlapping the layer or
 *     the mask in memory; per blit, in order, opacity > 255, invert > 1, then for w, h != 0 a rectangle that leaves the
 *     layer, one that leaves the mask.  FR_E_UNSUPPORTED: more than 2^22 tiles of 256 x 16 pixels.  FR_E_INVALID:
 *     overlapping clipped rectangles (the message names the first pair).  After any refusal the image is untouched.
 *     n_blits = 0 is valid and launches nothing, and so does a call whose blits all have o = 0.
 *   Execution: one launch of layer_mask_kernel<srgb, plane, erase> for all blits of the call, behind the small kernel that
 *     brings the call's tile table into device memory; invert and opacity are per-tile values.  A group of four pixels
 *     whose t are all 0, or whose layer pixels are all 0, is neither loaded from the destination nor stored; the
 *     destination is not loaded where every a' (erase: every t) is 255.  Asynchronous on the context's stream, in stream
 *     order with renders and the other layer calls; the caller may reuse `blits` as soon as the call returns.
 * FR_MASK_PLANE and FR_MASK_ERASE live in the flag space of the layer calls beside FR_LAYER_SRGB and FR_LCD_BGR, and only
 * fr_layer_mask knows them: the other layer calls refuse them as unknown bits.                                             */
#define FR_MASK_PLANE 4u   /* the mask is a plane of 1-byte elements (a coverage plan's output), any alignment */
#define FR_MASK_ERASE 8u   /* no source: the destination is multiplied by 255 - t (destination-out)           */

typedef struct fr_layer_mask_blit {
    uint32_t src_x, src_y;     /* top-left of the rectangle in the layer (ignored with FR_MASK_ERASE)  */
    uint32_t w, h;             /* 0 x anything: valid, does nothing                                    */
    int32_t  dst_x, dst_y;     /* where that top-left lands in the destination; may be negative        */
    uint32_t mask_x, mask_y;   /* the mask element that lies over the rectangle's top-left             */
    uint32_t opacity;          /* o in 0 .. 255                                                        */
    uint32_t invert;           /* 0: through the mask; 1: through its complement; else FR_E_INVALID    */
} fr_layer_mask_blit;

int fr_layer_mask(fr_ctx *ctx, const void *src_dev, size_t src_stride_px, size_t src_rows,
                  const void *mask_dev, size_t mask_stride, size_t mask_rows,
                  void *dst_dev, size_t dst_stride_px, size_t dst_rows,
                  const fr_layer_mask_blit *blits, uint32_t n_blits, uint32_t flags);

/* ---- a layer through an affine map: scaled, rotated and sub-pixel placement (BUILD-DEFINED; DESIGN.md sections 4.15 and 5) --
 * fr_layer_warp composites a premultiplied layer over a premultiplied image through an affine map, sampled bilinearly in
 * exact integers: a viewer that zooms, spins or smooth-scrolls finished text composites the layer per frame and does not
 * render the plan again.  Images, m, D, E, opacity, clipping, the non-overlap rule and the aliasing rule are
 * fr_layer_over's.  FR_LAYER_SRGB is the only known flag.
 *   Map: the caller gives the INVERSE map, destination to window.  A blit owns the dst_w x dst_h rectangle at (dst_x, dst_y)
 *     of the image and samples the w x h window at (src_x, src_y) of the layer.  For rectangle pixel (X, Y), 0 <= X < dst_w,
 *     0 <= Y < dst_h, in 1/65536 window pixel:
 *         U = u0 + X * ux + Y * uy,      V = v0 + X * vx + Y * vy
 *     exact integers that never wrap: |u0|, |v0| <= 2^47, dst_w, dst_h <= 2^26, the four coefficients any int32.  The centre
 *     of window pixel (i, j) is at ((i + 1/2) * 65536, (j + 1/2) * 65536).
 *   Taps: P = U - 32768, Q = V - 32768;  i = P >> 16, j = Q >> 16 (arithmetic shifts: floors);  fx = (P & 0xffff) >> 8,
 *     fy = (Q & 0xffff) >> 8 (0 .. 255: the fractions are truncated to 8 bits).  p(i, j) is window pixel (i, j) for
 *     0 <= i < w and 0 <= j < h and (0, 0, 0, 0) everywhere else.  No byte of the layer outside the window is ever read,
 *     whatever the map.
 *   Sample (UNORM), each of the four bytes c on its own:
 *         top = p(i, j)_c * (256 - fx) + p(i+1, j)_c * fx
 *         bot = p(i, j+1)_c * (256 - fx) + p(i+1, j+1)_c * fx
 *         s_c = (top * (256 - fy) + bot * fy + 32768) >> 16          (at most 255; the numerator fits 32 bits)
 *     and the pixel s is composited exactly as fr_layer_over composites a layer pixel at opacity o.
 *   Sample (FR_LAYER_SRGB): the alpha as above; the three colour bytes by the same formula on D[p_c], the 16-bit linear
 *     values (65535 * 65536 + 32768 < 2^32), giving S_c; the composite is fr_layer_over's sRGB line with S_c in the place
 *     of D[s_c]:
 *         out_c = E(min(65535, (S_c * o + 127) div 255 + (D[d_c] * (255 - a') + 127) div 255))
 *   Consequences:
 *     1. ux = vy = 65536, uy = vx = 0, u0 = 32768 + 65536 a, v0 = 32768 + 65536 b and a rectangle whose pixels stay inside
 *        the window: the bytes of fr_layer_over of that rectangle, at any o, in both spaces (fx = fy = 0, s = p).
 *     2. The eight quarter turns and mirrors in exact coefficients (+-65536 and 0) sample fx = fy = 0 everywhere: the bytes
 *        of fr_layer_over of the turned or mirrored layer.
 *     3. Where the four taps are equal the sample is that pixel; s lies between the smallest and the largest tap, per byte.
 *        A UNORM layer with s_c <= s_a everywhere gives samples with s_c <= s_a, so fr_layer_over's consequence 4 (no
 *        clamp) carries over.
 *     4. A shift of exactly half a pixel along one axis gives (p0 + p1 + 1) >> 1.
 *     5. A rectangle pixel whose four taps all lie outside the window is left byte-identical; so is any pixel under o = 0.
 *   Geometry: the rectangle is clipped to [0, dst_stride_px) x [0, dst_rows) as a blit of fr_layer_over is (X and Y keep
 *     counting from the unclipped corner); after clipping, the rectangles of one call must not overlap.  Inside a clipped
 *     rectangle any pixel may be read and written back unchanged; outside every clipped rectangle no byte of the image is
 *     touched.  A zero matrix is valid: every pixel samples one point.  w = 0 or h = 0 is valid and draws nothing.
 *   Validation, in this order.  FR_E_INVALID: NULL ctx; an unknown flag bit (FR_LCD_BGR, FR_MASK_PLANE and FR_MASK_ERASE
 *     are unknown here); a bad src, then a bad dst (NULL, not 4-byte aligned, a pitch above 2^26).  FR_E_UNSUPPORTED: 2^31
 *     rows or more in either image.  FR_E_INVALID: NULL blits with n_blits > 0; the two images overlapping in memory; per
 *     blit, in order, opacity > 255, reserved != 0, |u0| or |v0| above 2^47, dst_w or dst_h above 2^26, a window that
 *     leaves the layer (src_x + w > src_stride_px or src_y + h > src_rows).  FR_E_UNSUPPORTED: clipped rectangles that need
 *     more than 2^22 tiles of 32 x 32 pixels (counted before the culling below, blits with o = 0 or an empty window left
 *     out).  FR_E_INVALID: overlapping clipped rectangles.  After any refusal the image is untouched.  A call stages 96 bytes
 *     per listed tile in pinned host memory and in device memory, both kept by the context and grown by half as much again:
 *     0.8 MB for a 3840 x 2160 rectangle, and about 600 MB of each at the limit of 2^22 listed tiles (fr_layer_over: 200 MB);
 *     a call that cannot have them returns FR_E_HIP or FR_E_NOMEM with the image untouched.
 *   Execution: the host lists a 32 x 32 tile of a clipped rectangle only if the taps of some pixel of it can hit the window
 *     (U and V are affine, so their extremes sit at the tile's corners); a call that lists none launches nothing.  One
 *     launch of layer_warp_kernel<srgb, opacity> for all blits, behind the small kernel that brings the tile table into
 *     device memory; every lane gathers its taps from global memory.  Asynchronous on the context's stream, in stream
 *     order with renders and the other layer calls; the caller may reuse `blits` as soon as the call returns.            */
typedef struct fr_layer_warp_blit {
    uint32_t src_x, src_y, w, h;   /* the window of the layer that is sampled; must lie inside the layer        */
    int32_t  dst_x, dst_y;         /* top-left of the destination rectangle this blit owns; may be negative     */
    uint32_t dst_w, dst_h;         /* its size; 0 x anything is valid and does nothing                          */
    int64_t  u0, v0;               /* window position, 1/65536 pixel, sampled by the centre of rectangle pixel (0, 0) */
    int32_t  ux, uy, vx, vy;       /* its change per destination column (ux, vx) and row (uy, vy), 1/65536 pixel */
    uint32_t opacity;              /* o in 0 .. 255                                                             */
    uint32_t reserved;             /* must be 0                                                                 */
} fr_layer_warp_blit;              /* 72 bytes */

int fr_layer_warp(fr_ctx *ctx, const void *src_dev, size_t src_stride_px, size_t src_rows,
                  void *dst_dev, size_t dst_stride_px, size_t dst_rows,
                  const fr_layer_warp_blit *blits, uint32_t n_blits, uint32_t flags);

/* ---- blend modes: multiply, screen, overlay and the like (BUILD-DEFINED; DESIGN.md sections 4.16 and 5) --------------------
 * fr_layer_blend is fr_layer_over with a separable blend mode in the place of source-over: a highlighter stroke over text
 * (multiply), a glow (screen, plus), text that stays legible over light and dark (difference), a texture through a caption
 * (overlay).  The images (both premultiplied, alpha last), the blits with their geometry and clipping, the no-overlap
 * rules, the limits, the stream order and the promise that no byte outside a clipped rectangle is read or written are
 * fr_layer_over's, word for word; m, D and E as defined there.  One mode per call.  All integers.
 *   Definition: the W3C compositing formula co = cs (1 - ab) + cb (1 - as) + as ab B(Cb, Cs) on premultiplied values, with
 *   one rounding.  For a layer pixel (s_c, s_a), the destination pixel (d_c, d_a) under it, the blit's opacity o and
 *   a' = m(s_a, o), per colour byte c:
 *       flags = 0:      Q = 255,    x = m(s_c, o),                   p = a',      y = d_c,     q = d_a
 *       FR_LAYER_SRGB:  Q = 65535,  x = (D[s_c] * o + 127) div 255,  p = 257 a',  y = D[d_c],  q = 257 d_a
 *   and with (v)+ = max(0, v):
 *       N     = x (Q - q) + y (Q - p) + B2
 *       out   = min(Q, (N + (Q - 1) / 2) div Q)        stored as out_c = out (flags = 0) or E(out) (FR_LAYER_SRGB)
 *       out_a = a' + m(d_a, 255 - a')                  (fr_layer_over's alpha, in both spaces)
 *       B2:  FR_BLEND_MULTIPLY    x y
 *            FR_BLEND_SCREEN      (x q + y p - x y)+
 *            FR_BLEND_DARKEN      min(x q, y p)                 FR_BLEND_LIGHTEN    max(x q, y p)
 *            FR_BLEND_DIFFERENCE  |x q - y p|                   FR_BLEND_EXCLUSION  (x q + y p - 2 x y)+
 *            FR_BLEND_HARD_LIGHT  2 x <= p ?  2 x y  :  (p q - 2 (q - y)+ (p - x)+)+
 *            FR_BLEND_OVERLAY     2 y <= q ?  2 x y  :  (p q - 2 (q - y)+ (p - x)+)+
 *       FR_BLEND_PLUS (no N):  out = min(Q, x + y), stored likewise;  out_a = min(255, a' + d_a)
 *   Q is odd, so no ties occur.  The (.)+ and the final min make every byte combination defined, valid premultiplied or not.
 *   Consequences:
 *     1. For valid premultiplied inputs (x <= p, y <= q), N <= Q^2 and out is the integer nearest to the exact rational
 *        value of the W3C formula: the error is below 1/2 and never a tie.
 *     2. A layer pixel (0, 0, 0, 0), or o = 0, leaves the destination pixel byte-identical in every mode and both spaces.
 *     3. Over a destination pixel (0, 0, 0, 0) every mode gives fr_layer_over's bytes, for any layer bytes.
 *     4. MULTIPLY, SCREEN, DARKEN, LIGHTEN, DIFFERENCE, EXCLUSION and PLUS are symmetric in (layer, destination) at
 *        o = 255, for any bytes.
 *     5. HARD_LIGHT is OVERLAY with layer and destination swapped (at o = 255), for any bytes.
 *     6. For any bytes N never exceeds 3 Q^2 (MULTIPLY reaches it at x = y = Q, p = q = 0), which is above 2^32 in linear
 *        light: the kernel sums its 32-bit products in 64 bits.
 *   Not offered: colour-dodge, colour-burn and soft-light (a division or a square root per colour byte), the four
 *     non-separable modes (hue, saturation, colour, luminosity), a mode per blit, and blending through a mask or a warp:
 *     composite those into a cleared layer first (fr_layer_mask, fr_layer_warp) and blend that layer.
 *   Validation, in this order.  FR_E_INVALID: NULL ctx; an unknown flag bit (FR_LCD_BGR, FR_MASK_PLANE and FR_MASK_ERASE
 *     are unknown here); mode >= FR_BLEND_MODES; then everything fr_layer_over checks, in its order and with its codes.
 *     n_blits = 0 is valid and launches nothing.  After any refusal the image is untouched.
 *   Execution: one launch of layer_blend_kernel<srgb, mode, opacity> (opacity = 0 when every blit that draws has o = 255)
 *     over fr_layer_over's tiles of 256 x 16 pixels, behind the small kernel that brings the tile table into device memory.  A
 *     group of four layer pixels that are all zero is neither loaded from the image nor stored; every other pixel of a
 *     clipped rectangle needs its destination, opaque or not.  Asynchronous on the context's stream, in stream order with
 *     renders and the other layer calls; the caller may reuse `blits` as soon as the call returns.                        */
#define FR_BLEND_MULTIPLY   0u
#define FR_BLEND_SCREEN     1u
#define FR_BLEND_OVERLAY    2u
#define FR_BLEND_DARKEN     3u
#define FR_BLEND_LIGHTEN    4u
#define FR_BLEND_HARD_LIGHT 5u
#define FR_BLEND_DIFFERENCE 6u
#define FR_BLEND_EXCLUSION  7u
#define FR_BLEND_PLUS       8u
#define FR_BLEND_MODES      9u   /* the number of modes: mode >= FR_BLEND_MODES is FR_E_INVALID */

int fr_layer_blend(fr_ctx *ctx, const void *src_dev, size_t src_stride_px, size_t src_rows,
                   void *dst_dev, size_t dst_stride_px, size_t dst_rows,
                   const fr_layer_blit *blits, uint32_t n_blits, uint32_t mode, uint32_t flags);   /* 0 or FR_LAYER_SRGB */

/* ---- self-test: exhaustive device-side check of an arithmetic shortcut ----------
 * The render kernel computes t = num / d (render_glyph.zig:51,60-61; d an integer, |d| <= 2^17)
 * as a reciprocal multiply + FMA correction.  This compares that sequence with IEEE division
 * for EVERY binary32 significand and every integer divisor in [d_lo, d_hi] (both signs, three
 * binades) on the current HIP device; *mismatches must come back 0 for the shortcut to be
 * admissible.  The full range 1..131072 takes a few seconds.                              */
int fr_selftest_division(uint32_t d_lo, uint32_t d_hi, uint64_t *mismatches,
                         uint32_t *bad_divisor, uint32_t *bad_x_bits);
/* The render kernel's square root (delta of render_glyph.zig:60) skips the denormal pre-scaling of
 * the general lowering; this compares it with the correctly rounded sqrt for every binary32 in
 * [2^-30, 2^66) on the device.  *mismatches must come back 0.                                  */
int fr_selftest_sqrt(uint64_t *mismatches, uint32_t *bad_x_bits);
/* The row cuts of a glyph set (option "row_cuts") stand for the reference's acceptance test of a candidate root at a
 * ray height.  For every job, every candidate root of its glyph that the set-up does not discard from its control
 * points alone, and EVERY sample row of the job's cell (h * samples_per_axis rows at sample phase `phase`), this
 * compares on the device the class the cuts give with the class the acceptance expression gives, and once per job and
 * candidate the row range the set-up settles either way.  *pairs: the (candidate, row) pairs compared; *mismatches must
 * come back 0; first_bad (may be NULL, else three words): job, candidate (2 * segment of the glyph + root) and row of
 * the smallest mismatch, row 0xfffff meaning the settled ranges.  Jobs are checked as fr_plan_create checks them.  */
int fr_selftest_row_cuts(fr_glyphset *gs, const fr_job *jobs, uint32_t n_jobs, int samples_per_axis, int phase,
                         uint64_t *pairs, uint64_t *mismatches, uint32_t *first_bad);
/* The candidate table of a glyph set (option "cand_records") holds, per glyph, the records of its live candidate roots —
 * those the set-up does not discard from the control points alone and whose row cut is not empty — quadratic first,
 * linear last, each group in candidate order, and dead slots behind them.  For every glyph of the set this rebuilds each
 * candidate's record and cut on the device from the control points and compares with the table: the live count, the
 * order, every field bit for bit, and the dead slots' mark.  *live: the live candidates of the whole set; *mismatches
 * (slots that differ) must come back 0; first_bad (may be NULL, else two words): glyph and slot within the glyph of the
 * smallest mismatch; glyph_live (may be NULL, else one word per glyph): each glyph's live candidates as rebuilt.  */
int fr_selftest_cand_records(fr_glyphset *gs, uint64_t *live, uint64_t *mismatches, uint32_t *first_bad, uint32_t *glyph_live);

#ifdef __cplusplus
}
#endif
#endif /* FR_RASTER_H */

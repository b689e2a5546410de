// fr_internal.hpp — what the C ABI units (fr_api_*.hip) share: the three opaque structs of include/fr_raster.h, the views
// of device memory that launches read, and fail / HIP_TRY.  The units validate what the caller hands over, own device
// memory (DevBuf) and launch the kernels of the kernel units on the context's HIP stream.  No CPU rasterization path
// exists: without a usable gfx950 device every compute entry point returns FR_E_HIP.
#pragma once
#include "../../include/fr_raster.h"
#include "fr_devbuf.hpp"
#include "fr_device.hpp"
#include "fr_host_rules.hpp"
#include "fr_raster_plan.hpp"

#include <memory>
#include <vector>

namespace fr {
struct TextTile;                       // fr_text_tables.hpp
struct TextRun;
struct TextMaskCell;
struct TextMaskTile;
}  // namespace fr

// leaves the message for fr_last_error (this thread's) -> code
constexpr auto fail = fr::set_error;
#define HIP_TRY(expr)                                          \
    do {                                                       \
        hipError_t e_ = (expr);                                \
        if (e_ != hipSuccess) return hip_fail(e_, #expr);      \
    } while (0)

struct fr_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    bool owns_stream = false;
    uint32_t kmax = 32;          // crossings kept per sample row (register array: 8, 16 or 32) before the direct-sum fallback
    uint32_t strip_px = 256;     // column strip width, pixels (multiple of 16, <= 256)
    uint32_t fuse_prepare = 1;   // build root records inside the render kernel when every glyph has <= 128 segments
    uint32_t lds_pad = 0;        // experiment knob: extra dynamic LDS bytes per workgroup (occupancy studies)
    uint32_t min_wgs = 2048;     // split a cell's bands over workgroups below this many workgroups
    uint32_t cov4 = 1;           // jobs take the fast kernels (cov4_kernel / win1_kernel) where they fit (fast_class); 0: all general
    uint32_t row_cuts = 1;       // the fast kernels' set-up reads a row's class off the glyph set's row cuts; 0: evaluates the reference's acceptance
    uint32_t cand_records = 1;   // with row_cuts: the fast kernels' set-up reads each candidate's record from the glyph set's candidate table; 0: builds it from the control points
    uint32_t zero_copy = 0;      // fr_render_glyph: render small glyphs from / into pinned host memory directly (measured: no faster than two small copies; off)
    uint32_t sdf_cull = 1;       // FR_SDF_U8: drop segments that cannot change a tile / a pixel (exact; 0 = look at all, for tests)
    uint32_t overlap = 1;        // a plan's smaller launches run beside its largest one on a second stream: 0 never, 1 plans of >= 32 Mpixel, 2 always
    uint32_t graph = 0;          // 1: a plan's launches are captured into a hipGraph at its first render to a destination and replayed afterwards
    uint32_t opt_epoch = 0;      // moved by every successful fr_ctx_set_option of an option that feeds a launch: a captured graph is only
                                 // replayed under the options it was captured with
    hipStream_t aux = nullptr;   // that second stream and the fork / join events, created on first use
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    // scratch of the single-glyph entry point (fr_render_glyph): one device arena and one host staging
    // buffer, grown on demand and reused across calls
    DevBuf<unsigned char> arena;
    size_t arena_cap = 0;
    unsigned char *stage = nullptr;     // pinned host memory: [upload block | image coming back]
    size_t stage_cap = 0;
    // the tables of one fr_layer_over or fr_layer_rects call (fr_api_layer.hip): pinned host staging and the device copy the
    // kernel reads, room for layer_cap units of 16 bytes each, grown on demand; layer_ev: the last copy out of the staging
    // (layer_table_kernel), which the next call waits for
    DevBuf<uint4> layer_tab;
    uint4 *layer_stage = nullptr;
    size_t layer_cap = 0;
    hipEvent_t layer_ev = nullptr;
    // the two intermediate planes of fr_layer_shadow, one byte per pixel, grown on demand
    DevBuf<unsigned char> shadow_plane[2];
    size_t shadow_cap[2] = {0, 0};
};

// what kernels read of a glyph set
struct GlyphView {
    const int16_t *pts, *seg_pts;
    const uint32_t *seg_p0, *glyph_seg_start;
    fr::Rec *recs;                     // written by prepare_kernel
    uint32_t *rec_count;
    const float4 *seg_cut;             // may be null (RenderArgs::seg_cut)
    const uint4 *seg_cand;             // may be null (RenderArgs::seg_cand)
    uint32_t n_glyphs, max_seg_per_glyph;
};

struct fr_glyphset {
    fr_ctx *ctx = nullptr;
    uint32_t n_glyphs = 0, n_contours = 0, n_seg = 0, max_seg_per_glyph = 0;
    uint64_t n_points = 0;
    DevBuf<int16_t> pts, seg_pts;
    DevBuf<uint32_t> seg_p0, seg_prev, glyph_seg_start, rec_count;
    DevBuf<fr::Rec> recs;
    DevBuf<float4> seg_cut;                     // row cuts, one float4 per segment (fr_records.hpp): 16 B per segment
    DevBuf<uint4> seg_cand;                     // candidate table, two Cand per segment (fr_c4.hpp): 96 B per segment
    std::vector<uint32_t> h_glyph_seg_start;   // host copy: plans attach each job's segment range to it
    std::vector<uint32_t> h_root_bound;         // per glyph: candidate roots the vertex rule cannot discard (>= live records)
    std::vector<uint32_t> h_ray_bound;          // per glyph: estimated maximum of the crossings of one horizontal ray
    std::vector<int16_t> h_box;                 // fr_glyphset_set_boxes: Glyph.box per glyph (x_min, y_min, x_max, y_max); empty until set

    GlyphView view() const
    {
        return GlyphView{pts.get(), seg_pts.get(), seg_p0.get(), glyph_seg_start.get(), recs.get(), rec_count.get(), seg_cut.get(), seg_cand.get(), n_glyphs, max_seg_per_glyph};
    }
    ~fr_glyphset();                             // waits for the context's stream before the tables go
};

// what a raster plan's launches read besides the glyph set
struct RasterView {
    const fr::Job *jobs;
    const uint32_t *job_seg;           // [n_jobs][2]: first segment and segment count of the job's glyph
    const uint32_t *large;             // distinct glyphs of more than 128 segments among the general jobs (RasterPlan::n_large): their
                                       // records are rebuilt by prepare_kernel before every render (the others: inside the render kernel)
    uint32_t *bits;                    // FR_SDF_U8: the sign bit planes of the fast kernels' jobs (one bit per pixel: fr_win1.hip)
    const uint32_t *job_bits;          // and each job's first word in them (0xffffffff: a general-kernel job)
};

// the ten tables of a text plan
struct TextView {
    const fr::TextTile *tiles;
    const fr::TextRun *runs;
    const void *insts;                 // TextInst, TextInstEx or TextInstAffine (TextPlan::form); cached: TextCachedInst
    const uint32_t *list, *glyphs;     // the tiles' instance lists; the distinct glyphs whose records prepare_kernel rebuilds
    fr::Rec *recs;                     // into plan-owned memory before every render
    uint32_t *rec_count;
    // cached: a render fills the mask store from the cells' tiles between the prepare kernel and the composite
    const void *mcells;                // TextMaskCell; form TEXT_AFFINE: TextMaskCellAffine
    const fr::TextMaskTile *mtiles;
    uint16_t *masks;
};

// The launches of one raster render on the context's stream(s): the list of raster_launches over the two views.  A plan's
// render and fr_render_glyph (over its arena) both end here.
int raster_launch(fr_ctx *ctx, const GlyphView &g, const RasterView &r, const fr::RasterPlan &rp, const fr_raster_params &params,
                  uint32_t flags, void *out_dev, size_t out_stride);
fr::RasterOpts raster_opts(const fr_ctx *ctx);

// A plan: the head, and exactly one side (fr_api_plan.hip) that owns the tables and knows the launches.
struct RasterSide;
struct TextSide;
struct fr_plan {
    fr_ctx *ctx = nullptr;
    const fr_glyphset *gs = nullptr;
    fr_raster_params params{};
    uint32_t flags = 0;                // the create call's flags
    uint64_t pixels = 0, need_cols = 0, need_rows = 0;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    // option "graph": the launches of one render as an instantiated hipGraph, and what it was captured for
    hipGraphExec_t gexec = nullptr;
    void *g_out = nullptr;
    size_t g_stride = 0, g_rows = 0;
    uint32_t g_epoch = 0;
    std::unique_ptr<RasterSide> raster;
    std::unique_ptr<TextSide> text;

    fr_plan();
    ~fr_plan();                        // waits for the context's stream before the sides' tables go
};

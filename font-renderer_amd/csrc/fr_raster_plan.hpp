// fr_raster_plan.hpp — the host rules of a raster plan (fr_raster_plan.cpp): which kernel renders a job, the job order,
// the launch geometry, and the launches of one render as a list.  Plain C++: no HIP, no fr_ctx, no fr_plan.  fr_api.hip
// checks the caller's arguments, calls raster_plan_build, uploads what it returns, and walks raster_launches twice: to
// launch (plan_launch_direct) and to name (fr_plan_describe); host/raster_plan_selftest.cpp runs all of it on the CPU.
// A launch of the list names its kernel instance completely: the kernel units only look it up (pick, fr_device.hpp).
#pragma once
#include "../../include/fr_raster.h"

#include <cstddef>
#include <utility>
#include <vector>

namespace fr {

// record classes (128 / 256 / 512 / 1024 slots) x strip widths (64 / 128 / 256)
enum { FAST_RC = 4, FAST_CLASSES = 3 * FAST_RC };
// a plan's fast parts, the general launch with a prepare before and behind it, and the distance launch
enum { RASTER_MAX_LAUNCHES = FAST_CLASSES + 4 };
// segments of the largest glyph the fast kernels take (fr_cov4.hip: with 1024 record slots)
constexpr uint32_t COV4_MAX_SEGMENTS = 768u;

// the context options the rules read, and the waves of a workgroup of the general / the fast kernels
struct RasterOpts {
    uint32_t strip_px, cov4, fuse_prepare, min_wgs, overlap;
    uint32_t render_waves, fast_waves;
    uint32_t kmax;                     // crossings a sample row keeps: which CAP instance (raster_launches)
};

struct RasterPlanIn {
    const fr_job *jobs;                // checked by the caller (fr_plan_create_ex)
    uint32_t n_jobs;
    const uint32_t *glyph_seg_start;   // per glyph: first segment (n_glyphs + 1 entries), root bound and ray bound
    const uint32_t *root_bound, *ray_bound;
    fr_raster_params params;
    // what a plan does and the single-glyph call (fr_render_glyph) does not:
    bool sdf_fast;                     // FR_SDF_U8 jobs take win1_kernel's sign-bit mode where they fit, into a bit plane
    bool merge;                        // merge_small_classes
    bool uniform;                      // the general list may be `uniform` (false: never, whatever the cells' sizes)
};

// the tables of a plan in storage the caller provides: vectors for a plan, one element each on the stack for the
// single-glyph call
struct RasterTables {
    uint8_t *cls;                      // scratch: the job's class
    uint32_t *order;                   // sorted position -> index in RasterPlanIn::jobs: fast jobs first, grouped by class
    fr_job *sorted_jobs;
    uint32_t *jseg;                    // [n_jobs][2]: first segment and segment count of the job's glyph
    uint32_t *large;                   // the first n_large: distinct glyphs of more than 128 segments among the general jobs
    uint32_t *jbits;                   // with a bit plane: each job's first word in it (0xffffffff: a general-kernel job)
};

struct RasterPart { uint32_t first, cnt, wlog, rec_cap, bands, strips; uint64_t pixels; };

struct RasterPlan {
    uint32_t n_jobs = 0;
    // jobs cov4_kernel / win1_kernel take (fr_cov4.hip, fr_win1.hip): the first n_fast sorted jobs, grouped into `parts` —
    // one launch each, by strip width (64 / 128 / 256 pixels, from the job's own width) and by the record slots the glyph
    // needs (128 / 256 / 512 / 1024); the general kernel renders the other n_jobs - n_fast
    uint32_t n_fast = 0;
    RasterPart parts[FAST_CLASSES];
    uint32_t n_parts = 0;
    int fast_ns = 0;                   // samples per axis of the fast kernels' jobs (4 / 2: cov4_kernel, 1: win1_kernel)
    uint32_t strip_w = 0, gen_bands = 0, gen_strips = 0;   // the general launch
    bool uniform = false;              // see raster_plan_build
    uint32_t max_w = 0, max_h = 0;
    uint64_t pixels = 0, need_cols = 0, need_rows = 0;
    uint32_t n_large = 0;
    bool bit_plane = false;            // FR_SDF_U8 with fast jobs: jbits is filled, bit_words words of sign bits
    uint64_t bit_words = 0;            // (>= 2^32 - 1: more than a plan can address; jbits is not complete then)
    bool too_many = false;             // some launch needs more than 2^31 workgroups
};

// everything fr_plan_create computes before its first HIP call: t.cls, t.order and t.sorted_jobs (n_jobs entries each) and
// all of `p` but n_large and the bit plane
void raster_plan_build(const RasterPlanIn &in, const RasterOpts &opt, const RasterTables &t, RasterPlan &p);
// and what it computes beside the upload of the sorted jobs, unless p.too_many: t.jseg (2 n_jobs), t.large (room for
// n_jobs - n_fast) and, under FR_SDF_U8 with fast jobs, t.jbits (n_jobs); p.n_large, p.bit_plane, p.bit_words
void raster_plan_tables(const RasterPlanIn &in, const RasterTables &t, RasterPlan &p);

// fr_render_glyph's one job: the bounds of its own points, and not as a plan's: one SDF image takes its sign as a byte from
// the general kernel (no bit plane), there is no class to merge into, and the general kernel's instance is the ragged one
// whatever the image's size
inline RasterPlanIn single_glyph_in(const fr_job *jb, const uint32_t gseg[2], const uint32_t *root, const uint32_t *ray,
                                    const fr_raster_params &prm)
{
    RasterPlanIn in{};
    in.jobs = jb; in.n_jobs = 1; in.params = prm;
    in.glyph_seg_start = gseg; in.root_bound = root; in.ray_bound = ray;
    in.sdf_fast = false; in.merge = false; in.uniform = false;
    return in;
}

// ---- the launches of one render ----------------------------------------------------------------------------------
enum RasterFamily : uint8_t { RL_PREPARE, RL_RENDER, RL_COV4, RL_WIN1, RL_SDF };
struct RasterLaunch {
    RasterFamily family;
    bool uniform;
    bool largest;                      // the largest fast launch: it stays on the context's stream when the render forks
    // prepare: the fill flag.  render: the kernel's mode.  win1: 0 winding, 1 gray, 2 mask, 3 sign bits.  sdf: 1 = sdf_kernel<true>
    int mode;
    int samples;                       // per axis (render, cov4)
    uint32_t first, cnt;               // sorted jobs [first, first + cnt); prepare: cnt glyphs of `large`, 0 = the whole glyph set
    uint32_t strip_w, rec_cap, bands, strips, bands_per_wg, band_groups;
    // the kernel instance: its template arguments in the kernel's own order — cov4_kernel<WLOG, CAP, RPL, NS>,
    // win1_kernel<WLOG, MODE, RPL>, render_kernel<MODE, N, CAP, WLOG> (WLOG -1: the ragged one), sdf_kernel<bool> — and
    // whether it is the FILL twin.  Arguments the kernels have no instance of end the launch in hipErrorInvalidValue
    int targ[4];
    bool fill;
};
struct RasterLaunchList {
    RasterLaunch l[RASTER_MAX_LAUNCHES];
    uint32_t n = 0;
    uint32_t join_at = 0;              // launches [0, join_at) lie between the fork and the join, the rest behind the join
    bool forked = false;               // those go to the second stream, all but the largest fast one
};
// max_seg: segments of the glyph set's largest glyph (FR_SDF_U8: which distance kernel)
void raster_launches(const RasterPlan &p, const fr_raster_params &params, uint32_t flags, const RasterOpts &opt, uint32_t max_seg,
                     RasterLaunchList &out);
// the kernel of a render / cov4 / win1 / sdf launch as rocprofv3 names it, into name[cap] (a prepare launch: "")
void raster_launch_name(const RasterLaunch &e, char *name, size_t cap);

// one workgroup walks all bands of its cell unless the batch is too small to fill the chip: -> (bands per workgroup,
// workgroups per cell column)
std::pair<uint32_t, uint32_t> split_bands(uint32_t nw, uint32_t njobs, uint32_t bands, uint32_t strips, uint32_t min_wgs);

// ---- the rules, also called on their own (fr_glyphset_create, the exact path) ---------------------------------------
int flatten_segments(const uint32_t *contour_start, uint32_t n_contours, uint64_t *n_points, std::vector<uint32_t> &seg_p0,
                     std::vector<uint32_t> &seg_prev, std::vector<uint32_t> *contour_seg_start);
uint32_t glyph_root_bound(const int16_t *points_xy, const uint32_t *seg_p0, uint32_t s0, uint32_t s1);
uint32_t glyph_ray_bound(const int16_t *points_xy, const uint32_t *seg_p0, uint32_t s0, uint32_t s1,
                         std::vector<std::pair<int32_t, int32_t>> &ev);
struct FastRule {
    int ns = 0;             // samples per axis on the fast kernels (0: this plan has no fast kernel)
    uint32_t wlog_max = 0;  // widest strip the context allows (option "strip_px")
};
FastRule fast_rule(const RasterOpts &opt, const fr_raster_params *params);
int fast_class(const FastRule &R, uint32_t w, uint32_t h, uint32_t nsg, uint32_t root_bound, uint32_t ray_bound);
enum { FAST_PART_MIN = 64 };
void merge_small_classes(uint32_t counts[FAST_CLASSES], uint8_t *cls, uint32_t n_jobs);

int set_error(int code, const char *fmt, ...);   // fr_api.hip (the self-test has its own)

}  // namespace fr

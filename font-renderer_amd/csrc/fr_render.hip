// fr_render.hip — the hot path: per-pixel winding / analytic coverage of quadratic
// Bezier contours on gfx950 (wave64, LDS-staged, no MFMA: not a dense contraction).
//
// Replaces the O(W*H*S) loop of renderGlyph + glyphWindingAt
// (/root/reference/src/tools/render_glyph.zig:24-31, :35-73) with a formulation
// that yields the SAME integers:
//
//   winding(cx, cy) = sum over accepted roots k of  sign_k * [ not (xx_k < cx) ]   (:54,:66)
//
// where (xx_k, sign_k) depend only on the segment and the ROW (cy).  Per workgroup = (cell, group of
// wave bands, <= 256-px column strip), 4 waves; a wave band = 64 sample rows (64/N pixel rows):
//   set-up   every thread builds one candidate root record of the glyph straight into LDS, with the
//            EXACT range [ra, re) of this cell's sample rows on which the reference accepts it
//            (fr_records.hpp: the acceptance test is monotone in cy); the padded table of the exact
//            sample abscissae cx(j); ONE workgroup barrier.  Then the waves never meet again.
//   layout   per band, each lane clips the ranges of its 4 records to the band; one DPP prefix sum
//            places every record's run of (record, row) pairs in one sequence (marker at the run's
//            first slot) — no loop over records.
//   evaluate all 64 lanes take consecutive pairs (a DPP max-scan over the markers names the record):
//            t, xx, sign in the reference's own f32 operation order and its three acceptance tests,
//            J = #{sample columns j : cx(j) <= xx} against the table, append (J, step) to the row's
//            list in LDS.
//   sort     one lane per sample row: list -> registers (two 16-bit slots each), packed sorting network.
//   toggles  right to left with the running winding: a slot that changes zero <-> non-zero XORs a prefix
//            mask into the 64-bit LDS word of the 16-pixel window holding it (ds_xor_b64) and flips a
//            per-row "windows to my left are filled" parity word — O(crossings) per row.
//   windows  one lane per 16-pixel window: N mask words -> SWAR popcount per pixel -> 16 output bytes,
//            one 16-B store per lane (256 B per row run).
// Per-pixel work is O(crossings of its row), not O(segments).  A row with more than CAP crossings takes
// the direct sum over records (same integers, slower), inside the kernel.  DESIGN.md §3-§4 has the
// arguments and the measurements.
// Which instance a launch gets and how it is named is settled on the host, without HIP, by raster_launches and
// raster_launch_name (fr_raster_plan.cpp); launch_render at the end of this file only looks the instance up.
#include "fr_records.hpp"
#include "fr_wave.hpp"
#include "fr_raster_plan.hpp"

namespace fr {

enum { MODE_WINDING_I16 = 0, MODE_GRAY_DEBUG = 1, MODE_MASK_NONZERO = 2, MODE_COVERAGE_U8 = 3 };

__device__ __forceinline__ float bcast(float v, uint32_t k)
{
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), (int)k));
}

// One crossing = 16 bits: (J << 2) | code, J <= 1024 sample columns of a strip, winding step = code - 1
// (code 2: +1, code 0: -1).  An unused slot is 0xfffd: it sorts last and its step is 0, so the
// suffix sums and the toggle test need no "is this slot used" case.
constexpr uint32_t EMPTY = 0xfffdu;
constexpr uint32_t PCAP = 1024u;               // (record,row) pairs buffered per wave before a dense evaluation round
constexpr uint32_t LSTRIDE = 40u;              // u16 slots per row list: 32 used + pad; an 80-byte
                                               // row stride makes one-row-per-lane b128 reads conflict-free
constexpr uint32_t RCHUNK = 256u;              // records staged in LDS per pass
// waves per workgroup: they share one cell's records and cx table and take its wave bands round-robin
constexpr uint32_t NW = 4u;
constexpr uint32_t TAIL_BYTES = 64u * 4u;      // per-wave LDS tail: fill parity word of every sample row

// LDS line of sample row r (0..63 of a band) in a wave's window-mask array.  Swapping
// line parity with bit 2 puts rows r and r+4 (the same sub-row of two adjacent pixel rows,
// read together by one ds_read_b64 in phase 2) into different 128-B halves of the bank space.
__device__ __forceinline__ uint32_t mask_line(uint32_t r) { return r ^ ((r >> 2) & 1u); }
// 64-bit word of padding per mask line: without it every line starts in the same LDS bank and the toggles of a
// vertical edge (64 rows, same window) all hit one bank pair; with it consecutive lines are two banks apart
constexpr uint32_t MASK_PAD = 1u;

// WLOG >= 0: "uniform" plan — every strip of every job is exactly 16 << WLOG pixels wide and every
// job's height is a multiple of the wave band (RenderArgs::uniform, checked by fr_plan_create): strip
// width, window count and rows per band are compile-time constants (loop counts, addresses, no edge
// cases).  WLOG < 0: the general kernel.
// FILL: 0 (the reference's crossing rule) or 1 (FR_FILL_CONSISTENT: fr_records.hpp; the stand-alone records are then
// prepare_fill_kernel's).  Two kernel templates include the same body
// (the .inc file): render_kernel<3, 4, 32, -1> (the default instances keep
// their names and code) and render_kernel<3, 4, 32, -1, 1> — a __device__ body
// inlined into two wrapper kernels compiled the default instances to different code.
// Three workgroups fit a CU's LDS: the register allocation is held to three waves per SIMD (<= 168 VGPRs).
template <int MODE, int N, int CAP, int WLOG>
__global__ __launch_bounds__(64 * NW) __attribute__((amdgpu_waves_per_eu(3, 3))) void render_kernel(const RenderArgs A)
{
    constexpr int FILL = 0;
#include "fr_render_kernel.inc"
}
template <int MODE, int N, int CAP, int WLOG, int FILL>
__global__ __launch_bounds__(64 * NW) __attribute__((amdgpu_waves_per_eu(3, 3))) void render_kernel(const RenderArgs A)
{
#include "fr_render_kernel.inc"
}

// LDS plan: padded cx table | staged records [RCHUNK] | 4 x per-wave band region (window
// masks [64][nwin_pad + 1] u64, or breakpoint rows [64][CAP] u32) | 4 x fill[64]
void render_lds_plan(uint32_t strip_w, int n, int mode, uint32_t cap, uint32_t *nwin_log,
                     uint32_t *region, uint32_t *rec_bytes, uint32_t *wave_bytes, uint32_t *tail, size_t *total)
{
    uint32_t nwin = (strip_w + 15u) / 16u, lg = 0;
    while ((1u << lg) < nwin) ++lg;
    const size_t cx = (((size_t)strip_w * n + 2) * 4 + 15) & ~(size_t)15;
        size_t wb = mode == MODE_COVERAGE_U8 ? ((64u * ((1u << lg) + MASK_PAD) * 8u + 15u) & ~(size_t)15) : 64u * cap * 4;
    const size_t walk = 64u * LSTRIDE * 2u + PCAP * 2u + 64u * 8u + RCHUNK * 2u;   // lists, pairs / markers, cy, counters, run offsets
    if (wb < walk) wb = walk;                                  // the walk's buffers live here first
    const size_t rb = (size_t)RCHUNK * sizeof(Rec);
    const size_t t = cx + rb + NW * wb;
    *rec_bytes = (uint32_t)rb;
    *nwin_log = lg; *region = (uint32_t)cx; *wave_bytes = (uint32_t)wb; *tail = (uint32_t)t;
    *total = t + NW * TAIL_BYTES;
}

template <int MODE, int N, int CAP, int WLOG, int FILL>
static hipError_t launch_one(RenderArgs a, dim3 grid, hipStream_t stream)
{
    size_t lds;
    render_lds_plan(a.strip_w, N, MODE, CAP, &a.nwin_log, &a.lds_region, &a.lds_rec_bytes, &a.lds_wave_bytes, &a.lds_tail, &lds);
    lds += a.lds_pad;
    // (over-full rows are settled inside render_kernel)
    if constexpr (FILL) return launch_kernel(render_kernel<MODE, N, CAP, WLOG, 1>, grid, dim3(64 * NW), lds, stream, a);
    else return launch_kernel(render_kernel<MODE, N, CAP, WLOG>, grid, dim3(64 * NW), lds, stream, a);
}

// the (MODE, N, WLOG) triples render_kernel is compiled for, each with CAP 8 / 16 / 32 and both fill rules: coverage at
// 1, 2 and 4 samples per axis, winding and gray at one; only 4 x 4 coverage has the uniform instances (WLOG 4 / 3)
constexpr bool render_exists(int mode, int n, int wlog) { return mode == MODE_COVERAGE_U8 ? (wlog < 0 || n == 4) : (wlog < 0 && n == 1); }

uint32_t render_wg_waves() { return NW; }

// e.targ = MODE, N, CAP, WLOG
hipError_t launch_render(const RenderArgs &a, const RasterLaunch &e, hipStream_t stream)
{
    const dim3 grid((uint32_t)((size_t)a.n_jobs * a.band_groups * a.strips));
    if (a.strip_w == 0 || a.strip_w > 256u || (a.strip_w & 15u)) return hipErrorInvalidValue;
    const int key[] = {e.targ[0], e.targ[1], e.targ[2], e.targ[3], e.fill};
    return pick(key, [&](auto MODE, auto N, auto CAP, auto WLOG, auto FILL) -> hipError_t {
        if constexpr (render_exists(MODE, N, WLOG)) return launch_one<MODE, N, CAP, WLOG, FILL>(a, grid, stream);
        else return hipErrorInvalidValue;
    }, Among<MODE_WINDING_I16, MODE_GRAY_DEBUG, MODE_COVERAGE_U8>{}, Among<1, 2, 4>{}, Among<8, 16, 32>{}, Among<-1, 3, 4>{}, Among<0, 1>{});
}

}  // namespace fr

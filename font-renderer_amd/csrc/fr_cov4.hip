// fr_cov4.hip — the headline instance of the hot path: 16-sample (4 x 4; also 2 x 2) anti-aliased coverage of
// cells of any size, rebuilt around what bounds it on gfx950.  Same integers as render_kernel<COVERAGE_U8, 4> of
// fr_render.hip (and therefore as the reference's glyphWindingAt per sample,
// /root/reference/src/tools/render_glyph.zig:35-73, non-zero fill :29, box filter = the MSAA average
// resolve of VulkanContext.zig:307-313); a plan takes this kernel for every job it fits (any width and height up to
// 2048 sample rows, glyphs of <= 768 segments: fast_class, fr_raster_plan.cpp) and the general kernel for the rest.
// Which instance a launch gets and how it is named is settled on the host, without HIP, by raster_launches and
// raster_launch_name (fr_raster_plan.cpp); launch_cov4 at the end of this file only looks the instance up.
//
// What the round-2 measurements say (tools/ubench/issue_model*.hip, profiles/r02/issue_model*.txt):
// the path is bound by VECTOR-ALU ISSUE TIME — scalar, LDS and branch instructions of one wave hide under
// the vector instructions of the others.  A wave64 vector instruction holds its SIMD for ~4 cycles, except
// a "fast class" (VOP2 add/sub/and/or/xor/lshrrev/mov on VGPRs or literals, v_add_f32 / v_sub_f32 /
// v_mul_f32) that takes ~2 — but only with an EVEN number of waves per SIMD (at 3 waves/SIMD they cost
// 1.8x); v_sqrt_f32 ~7; a VOP2 v_cndmask whose VCC was not written by the instruction right before it
// ~10-19.  So this kernel (1) runs 4-wave workgroups, four per CU = 4 waves per SIMD; (2) turns the
// inside masks + transpose + popcount of the general kernel into signed byte DIFFERENCES of coverage that
// the window lanes integrate with a handful of fast adds (below); (3) keeps selects next to their compares
// or on SGPR masks; (4) drops work whose result is already known (the acceptance tests inside an exact
// row range).
//
// Coverage by integration.  For one sample row the inside set is a union of prefix intervals with signs:
//   inside(j) = sum_k sigma_k [j < J_k],  sigma_k = [w_left != 0] - [w_right != 0]  (non-zero rule)
// over the row's crossings sorted by J (w_right / w_left = winding right / left of crossing k).  The number
// of inside samples of pixel p (4 sample columns) from prefix [0, J) is clamp(J - 4p, 0, 4), i.e.
//   4 sigma + prefix-sum over q <= p of e[q],   e[P] = sigma (f - 4), e[P + 1] = -sigma f,  P = J >> 2, f = J & 3.
// Every toggle therefore adds two small signed numbers to a byte array E[pixel row][pixel] (LDS, ds_add_u32
// on the dword holding the bytes; bytes start at a bias of 16 so the final fields never borrow), the row's
// constant 4 [w(0) != 0] goes to byte 0, and a window lane (16 pixels of one pixel row) integrates: a
// multiply by 0x01010101 per dword, a 3-step chain across its 4 dwords, a 4-step DPP scan across the 16
// windows of the row — then maps 16 counts to bytes at once.  Integer all the way: the result is the same
// count k of inside samples per pixel, u8 = 16 k - [k > 8] = round_half_up(255 k / 16).
#include "fr_c4.hpp"
#include "fr_raster_plan.hpp"

namespace fr {

#ifdef FR_C4_STATS
__device__ unsigned long long g_c4_stats[16];
#endif
// Timing-only ablation builds (`make ablate4`, tools/c4_ablate.sh: wrong output by construction, never shipped) cut the
// kernel short at the C4_ABL_* points; their bodies live in fr_cov4_ablate.inc, which only those builds include.
#ifdef FR_C4_ABLATE
#include "fr_cov4_ablate.inc"
#else
#define C4_ABL_LAUNCH_ONLY()
#define C4_ABL_JOB_ONLY()
#define C4_ABL_SEGLOAD_ONLY()
#define C4_ABL_SETUP_ONLY()
#define C4_ABL_EVAL_ONLY()
#define C4_ABL_SORT_ONLY()
#define C4_ABL_KEEP(k) true
#define C4_ABL_NODECODE 0
#endif
// LDS plan (bytes): cx table | records | 8 x per-wave region | per-wave counters of the record compaction
template <int WLOG, int RPL, int NS, int CAP>
struct C4Lds {
    static constexpr uint32_t LSTRIDE = c4_lstride(CAP);
    static constexpr uint32_t NCOL = (16u << WLOG) * (uint32_t)NS;          // sample columns of a strip
    static constexpr uint32_t PRB = 64u / (uint32_t)NS;                     // pixel rows of a wave band (64 sample rows)
    static constexpr uint32_t CX = ((NCOL + 2u) * 4u + 15u) & ~15u;         // padded cx table
    static constexpr uint32_t RCAP = 64u * RPL;                             // root records a workgroup keeps
    static constexpr uint32_t REC = RCAP * (uint32_t)sizeof(Rec40);
    static constexpr uint32_t EROW = (16u << WLOG) + 16u;                   // bytes per pixel row of E (one 16-B pad)
    static constexpr uint32_t E = PRB * EROW;
    // walk buffers: lists [64][LSTRIDE] u16 | markers [PCAP] u16 | cy [64] f32 | cnt [64] u32 | roff [256] i16
    static constexpr uint32_t LISTS = 64u * LSTRIDE * 2u;
    static constexpr uint32_t OFF_PAIRS = LISTS;
    static constexpr uint32_t OFF_CY = OFF_PAIRS + C4_PCAP * 2u;
    static constexpr uint32_t OFF_CNT = OFF_CY + 256u;
    static constexpr uint32_t OFF_ROFF = OFF_CNT + 256u;
    static constexpr uint32_t WALK = OFF_ROFF + RCAP * 2u;
    // a row of 16-bit winding differences for an over-full sample row — only where 32 crossings are kept: the instances
    // that keep <= 16 settle such a row (one in 100 000 there) in registers and leave the LDS to two more workgroups per CU
    static constexpr uint32_t WD = (CAP <= 16) ? 0u : NCOL * 2u;
    static constexpr uint32_t WAVE = (WALK > E + WD ? WALK : E + WD);   // (E + an over-full row's 16-bit differences)
    static constexpr uint32_t OFF_WAVES = CX + REC;
    static constexpr uint32_t OFF_WCNT = OFF_WAVES + C4_WAVES * WAVE;
    static constexpr uint32_t TOTAL = OFF_WCNT + 64u;
};

// finished pixels of one 16-pixel window, clipped to the cell: the first m of the 16 bytes (m <= 0: none)
__device__ __forceinline__ void c4_store_clip(unsigned char *dst, uint4 v, int m)
{
    if (m >= 16) { c4_store16(dst, v); return; }
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int i = 0; i < 16; ++i)
        if (i < m) dst[i] = (unsigned char)(w[i >> 2] >> (8 * (i & 3)));
}

// One workgroup (4 waves) = one cell (or one group of its wave bands, or one strip of it).  The cell may be ragged:
// any width and height (renderGlyph sizes an image to the glyph's own box, render_glyph.zig:14-19) — the last strip
// and the last band are computed whole and their stores are clipped to the cell.
// WLOG: strip width 16 << WLOG pixels (2: 64, 3: 128, 4: 256).  CAP: crossings a sample row keeps (8 / 16 / 32);
// fuller rows take the direct sum over the glyph's records.  RPL: root records per lane, 2, 4 or 8 — a workgroup
// keeps up to 64 RPL records in LDS (128 / 256: four workgroups per CU; 512: three).  NS: samples per pixel axis,
// 4 (16 samples per pixel) or 2 (4): a wave band is 64 sample rows = 64 / NS pixel rows.
// FILL: 0 (the reference's crossing rule) or 1 (FR_FILL_CONSISTENT: fr_records.hpp).  Two kernel templates include the same body
// (the .inc file):
// cov4_kernel<4, 32, 4, 4> (the default instances keep their names and code) and cov4_kernel<4, 32, 4, 4, 1> — a __device__ body
// inlined into two wrapper kernels compiled the default instances to different code.
template <int WLOG, int CAP, int RPL, int NS>
__global__ __launch_bounds__(64 * C4_WAVES) __attribute__((amdgpu_waves_per_eu(c4_occ(CAP, WLOG, RPL), c4_occ(CAP, WLOG, RPL))))
void cov4_kernel(const RenderArgs A)
{
    constexpr int FILL = 0;
#include "fr_cov4_kernel.inc"
}
template <int WLOG, int CAP, int RPL, int NS, int FILL>
__global__ __launch_bounds__(64 * C4_WAVES) __attribute__((amdgpu_waves_per_eu(c4_occ(CAP, WLOG, RPL), c4_occ(CAP, WLOG, RPL))))
void cov4_kernel(const RenderArgs A)
{
#include "fr_cov4_kernel.inc"
}

#ifdef FR_C4_STATS
extern "C" int fr_debug_read_c4_stats(unsigned long long *out16, int reset)
{
    hipError_t e = hipMemcpyFromSymbol(out16, HIP_SYMBOL(g_c4_stats), sizeof(g_c4_stats));
    if (e == hipSuccess && reset) {
        unsigned long long z[16] = {0};
        e = hipMemcpyToSymbol(HIP_SYMBOL(g_c4_stats), z, sizeof z);
    }
    return e == hipSuccess ? 0 : -2;
}
#endif
uint32_t cov4_wg_waves() { return C4_WAVES; }
uint32_t cov4_max_segments() { return 768u; }     // (with 1024 record slots; 384 with 512, 256 for the smaller instances: fr_plan_create)

// FILL = 1: the FR_FILL_CONSISTENT twin of an instance (same launch shape and LDS)
template <int WLOG, int CAP, int RPL, int NS, int FILL>
static auto cov4_instance()
{
    if constexpr (FILL) return cov4_kernel<WLOG, CAP, RPL, NS, 1>;
    else return cov4_kernel<WLOG, CAP, RPL, NS>;
}

// the (CAP, RPL) pairs cov4_kernel is compiled for, each with every strip width, sample count and fill rule: the
// two-records-per-lane instances keep at most 16 crossings per sample row, the 1024-record one exists with 32 only
constexpr bool cov4_exists(int cap, int rpl) { return rpl == 16 ? cap == 32 : (rpl != 2 || cap <= 16); }

// jobs: cells of any size up to 2048 / ns sample rows (strips of a.strip_w in {64, 128, 256} pixels, wave bands of 64 / ns
// pixel rows; the last of each may be partial), ns x ns samples (ns in {2, 4}), every glyph with <= 384 segments and
// <= rec_cap (128, 256 or 512) possible root records (checked by fr_plan_create).  e.targ = WLOG, CAP, RPL, NS.
hipError_t launch_cov4(const RenderArgs &a, const RasterLaunch &e, hipStream_t stream)
{
    const dim3 grid((uint32_t)((size_t)a.n_jobs * a.band_groups * a.strips)), block(64 * C4_WAVES);
    const int key[] = {e.targ[0], e.targ[1], e.targ[2], e.targ[3], e.fill};
    return pick(key, [&](auto WLOG, auto CAP, auto RPL, auto NS, auto FILL) -> hipError_t {
        // (only the 512- and 1024-record instances need more than the default 48 KB)
        if constexpr (cov4_exists(CAP, RPL))
            return launch_kernel(cov4_instance<WLOG, CAP, RPL, NS, FILL>(), grid, block, C4Lds<WLOG, RPL, NS, CAP>::TOTAL + a.lds_pad, stream, a);
        else return hipErrorInvalidValue;
    }, Among<2, 3, 4>{}, Among<8, 16, 32>{}, Among<2, 4, 8, 16>{}, Among<2, 4>{}, Among<0, 1>{});
}

}  // namespace fr

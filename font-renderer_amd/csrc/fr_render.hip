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
#include "fr_records.hpp"
#include <cstdio>

namespace fr {

enum { MODE_WINDING_I16 = 0, MODE_GRAY_DEBUG = 1, MODE_MASK_NONZERO = 2, MODE_COVERAGE_U8 = 3 };

__device__ __forceinline__ uint32_t gray_debug(int w)
{
    int v = w * 20 + 100;                       // render_glyph.zig:28
    return (uint32_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

__device__ __forceinline__ float bcast(float v, uint32_t k)
{
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), (int)k));
}

// wave64 inclusive scans on DPP (row_shr within the 16-lane rows, then row_bcast:15 / :31 carry
// the row totals across rows): 6 VALU operations, no LDS.  `old` = 0 is the identity of both.
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ uint32_t dpp0(uint32_t x)
{
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, CTRL, ROW_MASK, 0xf, false);
}
__device__ __forceinline__ uint32_t wave_incl_add(uint32_t x)
{
    x += dpp0<0x111, 0xf>(x);                   // row_shr:1
    x += dpp0<0x112, 0xf>(x);                   // row_shr:2
    x += dpp0<0x114, 0xf>(x);                   // row_shr:4
    x += dpp0<0x118, 0xf>(x);                   // row_shr:8
    x += dpp0<0x142, 0xa>(x);                   // row_bcast:15 -> rows 1, 3
    x += dpp0<0x143, 0xc>(x);                   // row_bcast:31 -> rows 2, 3
    return x;
}
__device__ __forceinline__ uint32_t wave_incl_max(uint32_t x)
{
    x = max(x, dpp0<0x111, 0xf>(x));
    x = max(x, dpp0<0x112, 0xf>(x));
    x = max(x, dpp0<0x114, 0xf>(x));
    x = max(x, dpp0<0x118, 0xf>(x));
    x = max(x, dpp0<0x142, 0xa>(x));
    x = max(x, dpp0<0x143, 0xc>(x));
    return x;
}

#ifndef FR_BAND_PARTS
#define FR_BAND_PARTS 1
#endif
// One crossing = 16 bits: (J << 2) | code, J <= 1024 sample columns of a strip, winding step = code - 1
// (code 2: +1, code 0: -1).  An unused slot is 0xfffd: it sorts last and its step is 0, so the
// suffix sums and the toggle test need no "is this slot used" case.
constexpr uint32_t EMPTY = 0xfffdu;
constexpr uint32_t PCAP = 1024u;               // (record,row) pairs buffered per wave before a dense evaluation round
constexpr uint32_t LSTRIDE = 40u;              // u16 slots per row list: 32 used + pad; an 80-byte
                                               // row stride makes one-row-per-lane b128 reads conflict-free

// Sorting 2H crossings that sit PACKED two per register (d[j] = slot 2j | slot 2j+1 << 16), ascending:
//   1. Batcher's odd-even merge network over the H registers with v_pk_min_u16 / v_pk_max_u16 — the low
//      halves and the high halves are sorted as two independent sequences by the same instructions;
//   2. one "flip" step merges them (low[j] against high[H-1-j]; a half swap, a packed min/max and two
//      byte permutes per register pair): afterwards every low half <= every high half and both are bitonic;
//   3. log2(H) half-cleaner stages, again packed.
// Result: low halves = s[0..H), high halves = s[H..2H).  About half the instructions of the unpacked
// network, no unpacking, half the registers.
typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void pce(uint32_t &a, uint32_t &b)
{
    const u16x2 x = __builtin_bit_cast(u16x2, a), y = __builtin_bit_cast(u16x2, b);
    a = __builtin_bit_cast(uint32_t, __builtin_elementwise_min(x, y));
    b = __builtin_bit_cast(uint32_t, __builtin_elementwise_max(x, y));
}
template <int H>
__device__ __forceinline__ void packed_sort(uint32_t (&d)[16])
{
#pragma unroll
    for (int p = 1; p < H; p *= 2)
#pragma unroll
        for (int k = p; k >= 1; k /= 2)
#pragma unroll
            for (int j = k % p; j + k < H; j += 2 * k)
#pragma unroll
                for (int i = 0; i < k; ++i)
                    if (i + j + k < H && (i + j) / (2 * p) == (i + j + k) / (2 * p)) pce(d[i + j], d[i + j + k]);
#pragma unroll
    for (int j = 0; j < H / 2; ++j) {
        const uint32_t x = d[j], y = d[H - 1 - j];
        const uint32_t ys = __builtin_amdgcn_alignbit(y, y, 16);                    // halves swapped
        const u16x2 xv = __builtin_bit_cast(u16x2, x), yv = __builtin_bit_cast(u16x2, ys);
        const uint32_t mn = __builtin_bit_cast(uint32_t, __builtin_elementwise_min(xv, yv));
        const uint32_t mx = __builtin_bit_cast(uint32_t, __builtin_elementwise_max(xv, yv));
        d[j] = __builtin_amdgcn_perm(mx, mn, 0x05040100u);                          // min of pair j | max of pair j
        d[H - 1 - j] = __builtin_amdgcn_perm(mx, mn, 0x07060302u);                  // the same of pair H-1-j
    }
#pragma unroll
    for (int k = H / 2; k >= 1; k /= 2)
#pragma unroll
        for (int j = 0; j < H; ++j)
            if (!(j & k)) pce(d[j], d[j + k]);
}
// records staged in LDS per pass
#ifndef FR_RCHUNK
#define FR_RCHUNK 256
#endif
constexpr uint32_t RCHUNK = FR_RCHUNK;
// waves per workgroup: they share one cell's records and cx table and take its wave bands round-robin
#ifndef FR_WG_WAVES
#define FR_WG_WAVES 4
#endif
constexpr uint32_t NW = FR_WG_WAVES;
constexpr uint32_t TAIL_BYTES = (64u / FR_BAND_PARTS) * 4u;   // per-wave LDS tail: fill parity word of every sample row
// Diagnostic build only (make STAMPS=1 -> libfr_raster_stamps.so): per-phase shader-clock
// sums of wave 0 of every workgroup, added to a buffer nothing else reads.  The shipped
// library is built without FR_STAMPS and executes no stamp.
#ifdef FR_STAMPS
__device__ unsigned long long g_stamps[16];
#define STAMP(i)                                                                          \
    do {                                                                                  \
        __builtin_amdgcn_sched_barrier(0);                                                \
        unsigned long long t_;                                                            \
        asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory");        \
        __builtin_amdgcn_sched_barrier(0);                                                \
        acc_[i] += t_ - t_prev_;                                                          \
        t_prev_ = t_;                                                                     \
    } while (0)
#define STAMP_INIT()                                                                      \
    unsigned long long t_prev_, acc_[8] = {0, 0, 0, 0, 0, 0, 0, 0}, cacc_[4] = {0, 0, 0, 0}; \
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_prev_)::"memory")
// one atomic per phase per workgroup (wave 0), at the very end: the stamps themselves stay cheap
#define STAMP_FLUSH()                                                                     \
    do {                                                                                  \
        if (tid == 0)                                                                     \
            for (int i_ = 0; i_ < 8; ++i_) atomicAdd(&g_stamps[i_], acc_[i_]);            \
        if (lane == 0)                                                                    \
            for (int i_ = 0; i_ < 4; ++i_) atomicAdd(&g_stamps[8 + i_], cacc_[i_]);       \
    } while (0)
#define COUNT(i, n) do { cacc_[(i) - 8] += (unsigned long long)(n); } while (0)
#else
#define STAMP(i) do {} while (0)
#define STAMP_INIT() do {} while (0)
#define STAMP_FLUSH() do {} while (0)
#define COUNT(i, n) do {} while (0)
#endif

// LDS line of sample row r (0..31 of a half band) in a wave's window-mask array.  Swapping
// line parity with bit 2 puts rows r and r+4 (the same sub-row of two adjacent pixel rows,
// read together by one ds_read_b64 in phase 2) into different 128-B halves of the bank space.
#ifdef FR_NO_SWIZZLE
__device__ __forceinline__ uint32_t mask_line(uint32_t r) { return r; }
#else
__device__ __forceinline__ uint32_t mask_line(uint32_t r) { return r ^ ((r >> 2) & 1u); }
#endif
// 64-bit words of padding per mask line: with 0 every line starts in the same LDS bank and the toggles of a
// vertical edge (64 rows, same window) all hit one bank pair; 1 staggers consecutive lines by two banks
#ifndef FR_MASK_PAD
#define FR_MASK_PAD 1
#endif

// LDS hand-off inside ONE wave (writer lanes -> reader lanes of the same wave): LDS operations
// of a wave complete in order, so a drained lgkmcnt plus a compiler barrier is enough — no
// s_barrier, the other three waves of the workgroup are never waited for.
__device__ __forceinline__ void wave_lds_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// three workgroups fit a CU's LDS: hold the register allocation to three waves per SIMD (<= 168 VGPRs)
#ifndef FR_WAVES_PER_EU
#define FR_WAVES_PER_EU 3
#endif
#define FR_OCC __attribute__((amdgpu_waves_per_eu(FR_WAVES_PER_EU, FR_WAVES_PER_EU)))
// WLOG >= 0: "uniform" plan — every strip of every job is exactly 16 << WLOG pixels wide and every
// job's height is a multiple of the wave band (RenderArgs::uniform, checked by fr_plan_create): strip
// width, window count and rows per band are compile-time constants (loop counts, addresses, no edge
// cases).  WLOG < 0: the general kernel.
// FILL: 0 (the reference's crossing rule) or 1 (FR_FILL_CONSISTENT: fr_records.hpp; the stand-alone records are then
// prepare_fill_kernel's).  Two kernel templates include the same body
// (the .inc file): render_kernel<3, 4, 32, -1> (the default instances keep
// their names and code) and render_kernel<3, 4, 32, -1, 1> — a __device__ body
// inlined into two wrapper kernels compiled the default instances to different code.
template <int MODE, int N, int CAP, int WLOG>
__global__ __launch_bounds__(64 * FR_WG_WAVES) FR_OCC void render_kernel(const RenderArgs A)
{
    constexpr int FILL = 0;
#include "fr_render_kernel.inc"
}
template <int MODE, int N, int CAP, int WLOG, int FILL>
__global__ __launch_bounds__(64 * FR_WG_WAVES) FR_OCC void render_kernel(const RenderArgs A)
{
#include "fr_render_kernel.inc"
}

#ifdef FR_STAMPS
extern "C" int fr_debug_read_stamps(unsigned long long *out16, int reset)
{
    hipError_t e = hipMemcpyFromSymbol(out16, HIP_SYMBOL(g_stamps), sizeof(g_stamps));
    if (e == hipSuccess && reset) {
        unsigned long long z[16] = {0};
        e = hipMemcpyToSymbol(HIP_SYMBOL(g_stamps), z, sizeof z);
    }
    return e == hipSuccess ? 0 : -2;
}
#endif

// LDS plan: padded cx table | staged records [RCHUNK] | 4 x per-wave half-band region (window
// masks [32][nwin_pad] u64, or breakpoint rows [32][CAP] u32) | 4 x fill[32]
void render_lds_plan(uint32_t strip_w, int n, int mode, uint32_t cap, uint32_t *nwin_log,
                     uint32_t *region, uint32_t *rec_bytes, uint32_t *wave_bytes, uint32_t *tail, size_t *total)
{
    uint32_t nwin = (strip_w + 15u) / 16u, lg = 0;
    while ((1u << lg) < nwin) ++lg;
    const size_t cx = (((size_t)strip_w * n + 2) * 4 + 15) & ~(size_t)15;
    const size_t prow = 64u / FR_BAND_PARTS;
    size_t wb = mode == MODE_COVERAGE_U8 ? ((prow * ((1u << lg) + FR_MASK_PAD) * 8u + 15u) & ~(size_t)15) : prow * cap * 4;
    const size_t walk = 64u * LSTRIDE * 2u + PCAP * 2u + 64u * 8u + RCHUNK * 2u;   // lists, pairs / markers, cy, counters, run offsets
    if (wb < walk) wb = walk;                                  // the walk's buffers live here first
    const size_t rb = (size_t)RCHUNK * sizeof(Rec);
    const size_t t = cx + rb + NW * wb;
    *rec_bytes = (uint32_t)rb;
    *nwin_log = lg; *region = (uint32_t)cx; *wave_bytes = (uint32_t)wb; *tail = (uint32_t)t;
    *total = t + NW * TAIL_BYTES;
}

template <int MODE, int N, int CAP, int WLOG, int... FILLP>
static hipError_t launch_one(RenderArgs a, dim3 grid, hipStream_t stream, char *name, size_t name_cap)
{
    // as rocprofv3 names the instance
    if (name) snprintf(name, name_cap, sizeof...(FILLP) ? "fr::render_kernel<%d, %d, %d, %d, 1>" : "fr::render_kernel<%d, %d, %d, %d>", MODE, N, CAP, WLOG);
    if (!grid.x) return hipSuccess;                     // (name only)
    size_t lds;
    render_lds_plan(a.strip_w, N, MODE, CAP, &a.nwin_log, &a.lds_region, &a.lds_rec_bytes, &a.lds_wave_bytes, &a.lds_tail, &lds);
    lds += a.lds_pad;
    auto kern = render_kernel<MODE, N, CAP, WLOG, FILLP...>;
    if (lds > 48 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kern),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(kern, grid, dim3(64 * NW), lds, stream, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return hipSuccess;                                  // (over-full rows are settled inside render_kernel)
}

template <int MODE, int N, int WLOG, int... FILLP>
static hipError_t launch_cap_f(const RenderArgs &a, dim3 grid, hipStream_t stream, char *name, size_t name_cap)
{
    if (a.kmax <= 8) return launch_one<MODE, N, 8, WLOG, FILLP...>(a, grid, stream, name, name_cap);
    if (a.kmax <= 16) return launch_one<MODE, N, 16, WLOG, FILLP...>(a, grid, stream, name, name_cap);
    return launch_one<MODE, N, 32, WLOG, FILLP...>(a, grid, stream, name, name_cap);
}
// fill: the FR_FILL_CONSISTENT twin of every instance (same launch shape and LDS)
template <int MODE, int N, int WLOG>
static hipError_t launch_cap(const RenderArgs &a, dim3 grid, hipStream_t stream, char *name, size_t name_cap, int fill)
{
    if (fill) return launch_cap_f<MODE, N, WLOG, 1>(a, grid, stream, name, name_cap);
    return launch_cap_f<MODE, N, WLOG>(a, grid, stream, name, name_cap);
}

uint32_t render_wg_waves() { return NW; }

// launch = false: only name the instance (as rocprofv3 prints it) into `name`
hipError_t launch_render(const RenderArgs &a, int mode, int n, hipStream_t stream, bool launch, char *name, size_t name_cap, int fill)
{
    const dim3 grid(launch ? (uint32_t)((size_t)a.n_jobs * a.band_groups * a.strips) : 0u);
    if (a.strip_w == 0 || a.strip_w > 256u || (a.strip_w & 15u)) return hipErrorInvalidValue;
    if (mode == MODE_COVERAGE_U8) {
        if (n == 1) return launch_cap<MODE_COVERAGE_U8, 1, -1>(a, grid, stream, name, name_cap, fill);
        if (n == 2) return launch_cap<MODE_COVERAGE_U8, 2, -1>(a, grid, stream, name, name_cap, fill);
        if (n == 4) {
            // uniform plans of 256- / 128-pixel strips (atlas cells) take the specialised instances
            if (a.uniform && a.strip_w == 256u) return launch_cap<MODE_COVERAGE_U8, 4, 4>(a, grid, stream, name, name_cap, fill);
            if (a.uniform && a.strip_w == 128u) return launch_cap<MODE_COVERAGE_U8, 4, 3>(a, grid, stream, name, name_cap, fill);
            return launch_cap<MODE_COVERAGE_U8, 4, -1>(a, grid, stream, name, name_cap, fill);
        }
        return hipErrorInvalidValue;
    }
    if (n != 1) return hipErrorInvalidValue;
    if (mode == MODE_WINDING_I16) return launch_cap<MODE_WINDING_I16, 1, -1>(a, grid, stream, name, name_cap, fill);
    if (mode == MODE_GRAY_DEBUG) return launch_cap<MODE_GRAY_DEBUG, 1, -1>(a, grid, stream, name, name_cap, fill);
    // winding != 0 ? 255 : 0 is exactly the 1-sample coverage (round_half_up(255 k / 1), k in {0, 1})
    if (mode == MODE_MASK_NONZERO) return launch_cap<MODE_COVERAGE_U8, 1, -1>(a, grid, stream, name, name_cap, fill);
    return hipErrorInvalidValue;
}

}  // namespace fr

// fr_win1.hip — the reference's own products at one sample per pixel: Image.Winding (int16 winding numbers),
// renderGlyph's gray map clamp(w * 20 + 100) (/root/reference/src/tools/render_glyph.zig:28) and the non-zero mask
// (:29), for cells of any width and height (renderGlyph's own image sizes included, :14-19) of glyphs of <= 768
// segments; the general render_kernel keeps the rest.
//
// Same integers as glyphWindingAt per pixel (:35-73): winding(x) = sum over accepted roots of step [x < J].
// With one sample per pixel there is no inside/outside rule to apply per sample row, so nothing has to be sorted:
// every crossing subtracts its step from ONE byte of a row of winding DIFFERENCES (LDS, ds_add_u32 on the dword
// holding it) straight from the evaluation — w(x) = w(0) - sum over the crossings with J <= x of their step, byte J
// takes - step, and w(0) = the sum of all steps rides in the high half of the row's crossing counter (one more
// ds_add_u32 that the count needs anyway) — and a window lane integrates 16 pixels exactly as cov4_kernel
// integrates coverage (multiply by 0x01010101 per dword, 3-step chain, 4-step DPP scan across the 16 windows of a
// row), in pixel order.  Bytes carry a bias (32 in LDS, 96
// after the scans) and hold |w| <= 31: a row with more than 31 crossings (it alone could leave that range) takes
// the direct path — 16-bit differences, suffix scan, pixels written from there.  No lists, no sort, no toggles:
// per 4 KB of gray output about half the vector instructions of cov4_kernel's 16-sample pixel.
// Which instance a launch gets and how it is named is settled on the host, without HIP, by raster_launches and
// raster_launch_name (fr_raster_plan.cpp); launch_win1 at the end of this file only looks the instance up.
#include "fr_c4.hpp"
#include "fr_raster_plan.hpp"

namespace fr {

// MODE1_BITS: the non-zero mask as ONE BIT per pixel in job-local bit planes (A.out = the planes' base, A.job_bits[j] =
// the job's first 32-bit word) — the sign the SDF kernel reads (fr_sdf.hip): an eighth of the bytes of the mask, and
// the output itself is then written only once.  Layout: one plane per 256-pixel column of the cell, ceil(w / 256) of
// them one after the other, each h rows of 8 words (bit x % 32 of word (x % 256) / 32 = pixel x) — so the 16 rows of a
// band of a 256-pixel strip are 512 CONTIGUOUS bytes, which leave as 32 lanes x 16 bytes in one store instruction.
// (Measured, WRITE_SIZE per launch for 16.8 MB of bit planes: rows of ceil(w / 32) words written 2 bytes per window
// 76 MB; this layout written 2 bytes per window 49 MB, 16 bytes per every eighth lane 112 MB, whole 512-byte runs 23 MB;
// one plane per 64-pixel column in whole 128-byte lines 76 MB.)
enum { MODE1_WINDING_I16 = 0, MODE1_GRAY_DEBUG = 1, MODE1_MASK = 2, MODE1_BITS = 3 };
enum { W1_ROWS = 16 };

template <int WLOG, int RPL>
struct W1Lds {
    static constexpr uint32_t NCOL = 16u << WLOG;                           // sample columns = pixels of a strip
    static constexpr uint32_t CX = ((NCOL + 2u) * 4u + 15u) & ~15u;
    static constexpr uint32_t RCAP = 64u * RPL;
    static constexpr uint32_t REC = RCAP * (uint32_t)sizeof(Rec40);
    // pairs per round (one row has <= RCAP).  The two-records-per-lane instances take 128 and settle an over-full row in
    // registers (below) instead of in the marker array: that is what lets SIX of their workgroups share a CU at 256-pixel strips
    static constexpr uint32_t PCAP = RCAP > 256u ? RCAP : (RPL == 2 ? 128u : 256u);
    static constexpr bool WD_LDS = RPL != 2;                                // an over-full row's 16-bit differences live in the marker array
    static constexpr uint32_t EROW = NCOL + 16u;
    static constexpr uint32_t E = W1_ROWS * EROW;
    // per wave: E | markers [PCAP] u16 (later: one row of 16-bit differences) | cy [16] | cnt [16] | roff [RCAP] i16
    static constexpr uint32_t OFF_PAIRS = E;
    static constexpr uint32_t OFF_CY = OFF_PAIRS + PCAP * 2u;
    static constexpr uint32_t OFF_CNT = OFF_CY + 64u;
    static constexpr uint32_t OFF_ROFF = OFF_CNT + 64u;
    static constexpr uint32_t WAVE = (OFF_ROFF + RCAP * 2u + 15u) & ~15u;
    static constexpr uint32_t OFF_WAVES = CX + REC;
    static constexpr uint32_t OFF_WCNT = OFF_WAVES + C4_WAVES * WAVE;
    static constexpr uint32_t OFF_CYT = OFF_WCNT + 64u;                     // ray heights of the cell's rows (cells of <= 256 rows)
    static constexpr uint32_t TOTAL = OFF_CYT + 1024u;
};

// the first m of a window's 16 pixels (m <= 0: none), ESZ bytes each: a (and b, the second half of 16 int16 values)
template <uint32_t ESZ>
__device__ __forceinline__ void w1_store_clip(unsigned char *dst, uint4 a, uint4 b, int m)
{
    if (m >= 16) {
        if (ESZ == 2u) { __builtin_memcpy(dst, &a, 16); __builtin_memcpy(dst + 16, &b, 16); }
        else c4_store16(dst, a);
        return;
    }
    const uint32_t w[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        if (i >= m) continue;
        if (ESZ == 2u) reinterpret_cast<uint16_t *>(dst)[i] = (uint16_t)(w[i >> 1] >> (16 * (i & 1)));
        else dst[i] = (unsigned char)(w[i >> 2] >> (8 * (i & 3)));
    }
}

// Sign bits of one row of a narrow strip (64 / 128 pixels) or of a row the direct path settled: lane `wx` of the row's
// consecutive lanes holds the 16 bits of its window; four windows are gathered across the lanes and stored as 8 bytes by
// every fourth lane.  Every lane of the wave must call this (the gather reads its neighbours); `row` = the first byte of
// the strip's part of the row in the bit plane, `ok` = the row lies in the cell.
template <int WLOG>
__device__ __forceinline__ void w1_store_bits(unsigned char *row, uint32_t wx, uint32_t bits16, bool ok)
{
    const uint32_t pair = bits16 | ((uint32_t)__shfl_down((int)bits16, 1) << 16);           // windows wx, wx + 1 (even wx)
    const uint32_t d1 = (uint32_t)__shfl_down((int)pair, 2);
    if (ok && (wx & 3u) == 0u) { const uint2 v = make_uint2(pair, d1); __builtin_memcpy(row + 2u * wx, &v, 8); }
}

// FILL: 0 (the reference's crossing rule) or 1 (FR_FILL_CONSISTENT: fr_records.hpp).  Two kernel templates include the same body
// (the .inc file):
// win1_kernel<4, 2, 2> (the default instances keep their names and code) and win1_kernel<4, 2, 2, 1> — a __device__ body
// inlined into two wrapper kernels compiled the default instances to different code.
template <int WLOG, int MODE, int RPL>
__global__ __launch_bounds__(64 * C4_WAVES) __attribute__((amdgpu_waves_per_eu(w1_occ(RPL, WLOG), w1_occ(RPL, WLOG))))
void win1_kernel(const RenderArgs A)
{
    constexpr int FILL = 0;
#include "fr_win1_kernel.inc"
}
template <int WLOG, int MODE, int RPL, int FILL>
__global__ __launch_bounds__(64 * C4_WAVES) __attribute__((amdgpu_waves_per_eu(w1_occ(RPL, WLOG), w1_occ(RPL, WLOG))))
void win1_kernel(const RenderArgs A)
{
#include "fr_win1_kernel.inc"
}

uint32_t win1_band_rows() { return W1_ROWS; }

// FILL = 1: the FR_FILL_CONSISTENT twin of an instance (same launch shape and LDS)
template <int WLOG, int MODE, int RPL, int FILL>
static auto win1_instance()
{
    if constexpr (FILL) return win1_kernel<WLOG, MODE, RPL, 1>;
    else return win1_kernel<WLOG, MODE, RPL>;
}

// jobs: cells of any size up to 2048 rows (strips of a.strip_w in {64, 128, 256} pixels and bands of 16 rows; the last of
// each may be partial), one sample per pixel, glyphs with <= 384 segments and <= rec_cap possible root records.
// e.targ = WLOG, MODE (0 winding_i16, 1 gray_debug, 2 mask, 3 sign bits: one per pixel, job-local bit plane), RPL.
hipError_t launch_win1(const RenderArgs &a, const RasterLaunch &e, hipStream_t stream)
{
    const dim3 grid((uint32_t)((size_t)a.n_jobs * a.band_groups * a.strips)), block(64 * C4_WAVES);
    const int key[] = {e.targ[0], e.targ[1], e.targ[2], e.fill};
    return pick(key, [&](auto WLOG, auto MODE, auto RPL, auto FILL) {
        return launch_kernel(win1_instance<WLOG, MODE, RPL, FILL>(), grid, block, W1Lds<WLOG, RPL>::TOTAL + a.lds_pad, stream, a);
    }, Among<2, 3, 4>{}, Among<MODE1_WINDING_I16, MODE1_GRAY_DEBUG, MODE1_MASK, MODE1_BITS>{}, Among<2, 4, 8, 16>{}, Among<0, 1>{});
}

}  // namespace fr

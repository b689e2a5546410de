// fr_selftest.hip — exhaustive on-device proof obligations for arithmetic shortcuts.
//
// div_by_int (fr_device.hpp) replaces the IEEE division  t = num / d  of
// /root/reference/src/tools/render_glyph.zig:51,60-61 by a reciprocal multiply plus Markstein's
// FMA correction.  That is only admissible if it returns the SAME binary32 for every input the
// render kernel can feed it.  d is an integer (a = p0y - 2 p1y + p2y, or p2y - p0y) with
// |d| <= 4*32768 = 2^17.  This kernel checks, for every integer d in [d_lo, d_hi] and EVERY one
// of the 2^23 significands x in [1, 2) — plus the same significands at two other binades and
// with both signs of d — that div_by_int(x, d, RN(1/d)) == x / d bit for bit (hipcc's default
// correctly-rounded division).  Scaling x by 2^k is exact for q, r and q', so one binade
// represents them all while every intermediate stays normal.
#include "../../include/fr_raster.h"
#include "fr_c4.hpp"

namespace fr {

__global__ __launch_bounds__(256) void selftest_div_kernel(uint32_t d_lo, uint32_t n_d,
                                                           unsigned long long *mismatches,
                                                           uint32_t *first_bad)
{
    const uint32_t d_idx = blockIdx.x / 32u, part = blockIdx.x % 32u;
    if (d_idx >= n_d) return;
    const float d = (float)(d_lo + d_idx);
    const float rd = 1.0f / d, rdn = 1.0f / (-d);
    uint32_t bad = 0, bad_x = 0;
    // 2^23 significands split over 32 blocks x 256 threads
    for (uint32_t m = part * 256u + threadIdx.x; m < (1u << 23); m += 32u * 256u) {
        const float x = __uint_as_float(0x3f800000u | m);               // [1, 2)
        const float xs = __uint_as_float(0x2f800000u | m);              // [2^-32, 2^-31)
        const float xl = __uint_as_float(0x4f800000u | m);              // [2^32, 2^33)
        const bool ok = (__float_as_uint(div_by_int(x, d, rd)) == __float_as_uint(x / d)) &&
                        (__float_as_uint(div_by_int(x, -d, rdn)) == __float_as_uint(x / -d)) &&
                        (__float_as_uint(div_by_int(-xs, d, rd)) == __float_as_uint(-xs / d)) &&
                        (__float_as_uint(div_by_int(xl, d, rd)) == __float_as_uint(xl / d));
        if (!ok) { ++bad; bad_x = 0x3f800000u | m; }
    }
    if (bad) {
        atomicAdd(mismatches, (unsigned long long)bad);
        atomicMax(&first_bad[0], d_lo + d_idx);
        first_bad[1] = bad_x;
    }
}

// sqrt_rn (fr_device.hpp) == the correctly rounded square root for every binary32 whose exponent
// field lies in [e_lo, e_hi] (positive, normal): one block row per exponent, all 2^23 significands.
__global__ __launch_bounds__(256) void selftest_sqrt_kernel(uint32_t e_lo, unsigned long long *mismatches, uint32_t *first_bad)
{
    const uint32_t e = e_lo + blockIdx.x / 32u, part = blockIdx.x % 32u;
    uint32_t bad = 0, bad_x = 0;
    for (uint32_t m = part * 256u + threadIdx.x; m < (1u << 23); m += 32u * 256u) {
        const uint32_t bits = (e << 23) | m;
        const float x = __uint_as_float(bits);
        if (__float_as_uint(sqrt_rn(x)) != __float_as_uint(__builtin_sqrtf(x))) { ++bad; bad_x = bits; }
    }
    if (bad) {
        atomicAdd(mismatches, (unsigned long long)bad);
        first_bad[0] = bad_x;
    }
}

// the same sweep for the candidate sqrt_fast<VARIANT> (fr_device.hpp); thread 0 of block 0 also takes the two special
// arguments: 0 must give 0 and a negative number a NaN, as sqrt_rn does
template <int VARIANT>
__global__ __launch_bounds__(256) void selftest_sqrt_fast_kernel(uint32_t e_lo, unsigned long long *mismatches, uint32_t *first_bad)
{
    const uint32_t e = e_lo + blockIdx.x / 32u, part = blockIdx.x % 32u;
    uint32_t bad = 0, bad_x = 0;
    for (uint32_t m = part * 256u + threadIdx.x; m < (1u << 23); m += 32u * 256u) {
        const uint32_t bits = (e << 23) | m;
        const float x = __uint_as_float(bits);
        if (__float_as_uint(sqrt_fast<VARIANT>(x)) != __float_as_uint(__builtin_sqrtf(x))) { ++bad; bad_x = bits; }
    }
    if (blockIdx.x == 0u && threadIdx.x == 0u) {
        // (opaque: the compiler must not fold the candidate at these two arguments)
        float z = 0.0f, n = -2.0f;
        asm volatile("" : "+v"(z), "+v"(n));
        if (__float_as_uint(sqrt_fast<VARIANT>(z)) != 0u) { ++bad; bad_x = 0u; }
        const float sn = sqrt_fast<VARIANT>(n);
        if (sn == sn) { ++bad; bad_x = __float_as_uint(n); }
    }
    if (bad) {
        atomicAdd(mismatches, (unsigned long long)bad);
        first_bad[0] = bad_x;
    }
}

// The glyph set's row cuts (fr_records.hpp) against the expression they stand for, over the cells of `jobs`.
// Block (j, chunk): job j, sample rows [64 chunk, 64 chunk + 64) of its cell; thread t takes candidates t, t + 256, ...
// of the job's glyph that record_prep does not discard, and for each compares classify_cut with classify_row at every
// row of the chunk.  Chunk 0 also settles each candidate's row range both ways from the same guess — and, as the
// set-ups do, takes a cut that misses the cell's heights for an empty range — and compares the two.
// res[0]: (candidate, row) pairs compared, res[1]: mismatches, res[2]: the smallest mismatch as
// job << 40 | candidate << 20 | row (row 0xfffff: the settled ranges differ).
__global__ __launch_bounds__(256) void selftest_row_cuts_kernel(const Job *__restrict__ jobs, const uint32_t *__restrict__ glyph_seg_start,
                                                                const int16_t *__restrict__ seg_pts, const float4 *__restrict__ seg_cut,
                                                                int n, int phase, unsigned long long *res)
{
    const uint32_t j = blockIdx.x, row0 = blockIdx.y * 64u;
    const Job job = jobs[j];
    const uint32_t rows = job.h * (uint32_t)n;
    if (row0 >= rows) return;
    const uint32_t row1 = min(row0 + 64u, rows);
    const uint32_t seg0 = glyph_seg_start[job.glyph], n_cand = 2u * (glyph_seg_start[job.glyph + 1u] - seg0);
    RowGeom geo;
    geo.max_y = job.max_y; geo.set_scale(scale_div(job.scale)); geo.rows = rows; geo.n = n; geo.phase = phase;
    const RowSpan span = row_span(geo);
    unsigned long long pairs = 0ull, bad = 0ull, first = ~0ull;
    for (uint32_t c = threadIdx.x; c < n_cand; c += 256u) {
        Rec r;
        RowGuess g;
        record_prep<0>(seg_pts + 6u * (size_t)(seg0 + (c >> 1)), c & 1u, geo, r, g);
        if (g.empty) continue;
        const float2 q = reinterpret_cast<const float2 *>(seg_cut)[2u * (size_t)seg0 + c];
        Cut k;
        k.lo = q.x; k.hi = q.y;
        const unsigned long long where = ((unsigned long long)j << 40) | ((unsigned long long)min(c, 0xfffffu) << 20);
        for (uint32_t row = row0; row < row1; ++row) {
            const float cy = geo.cy(row);
            ++pairs;
            if (classify_cut(k, cy) != classify_row(r, cy)) { ++bad; first = min(first, where | row); }
        }
        if (row0 == 0u) {
            uint32_t ra0 = g.ra, re0 = g.re, ra1 = g.ra, re1 = g.re;
            record_settle<0, 0>(r, geo, ra0, re0);
            record_settle<0, 1>(r, geo, ra1, re1, nullptr, &k);
            bool differ = ra0 != ra1 || re0 != re1;
            if (cut_misses(k, span)) differ = differ || ra0 < re0;
            if (differ) { ++bad; first = min(first, where | 0xfffffull); }
        }
    }
    if (pairs) atomicAdd(&res[0], pairs);
    if (bad) { atomicAdd(&res[1], bad); atomicMin(&res[2], first); }
}

// jobs: device memory.  max_rows: the largest h * n among them.  res: three zero-initialised (res[2]: all ones) words
void launch_selftest_row_cuts(const Job *jobs, uint32_t n_jobs, uint32_t max_rows, const uint32_t *glyph_seg_start, const int16_t *seg_pts,
                              const float4 *seg_cut, int n, int phase, unsigned long long *res, hipStream_t stream)
{
    if (n_jobs == 0 || max_rows == 0) return;
    hipLaunchKernelGGL(selftest_row_cuts_kernel, dim3(n_jobs, (max_rows + 63u) / 64u), dim3(256), 0, stream, jobs, glyph_seg_start,
                       seg_pts, seg_cut, n, phase, res);
}

// The glyph set's candidate table (Cand, fr_c4.hpp) against what it stands for.  One wave per glyph: lane l rebuilds
// candidates l, l + 64, ... from the control points (record_prep, then find_cut — not the stored cuts), and the wave
// works out where each live one belongs: quadratic first, linear last, each group in candidate order.  The slot there
// must hold the rebuilt record and cut bit for bit (all twelve words), and every slot behind the live ones must be a
// dead one: a == 0 and the empty cut.  That is the live count, the order, every field and the dead marks at once.
// res[0]: live candidates, res[1]: mismatching slots, res[2]: the smallest mismatch as glyph << 32 | slot;
// glyph_live[g]: the live candidates of glyph g as rebuilt.
__global__ __launch_bounds__(64) void selftest_cand_records_kernel(const uint32_t *__restrict__ glyph_seg_start, const int16_t *__restrict__ seg_pts,
                                                                   const Cand *__restrict__ tab, uint32_t n_glyphs, unsigned long long *res,
                                                                   uint32_t *__restrict__ glyph_live)
{
    const uint32_t gl = blockIdx.x, lane = threadIdx.x;
    if (gl >= n_glyphs) return;
    const uint32_t s0 = glyph_seg_start[gl], n_cand = 2u * (glyph_seg_start[gl + 1u] - s0);
    const size_t base = 2u * (size_t)s0;
    RowGeom G;                                     // (no cell: record_prep's row guesses are not used)
    G.max_y = 0; G.scale = 1.0f; G.rows = 0u; G.n = 1; G.phase = 0;
    const unsigned long long below = (1ull << lane) - 1ull;
    // walk 0 counts the live quadratic candidates, walk 1 compares
    uint32_t n_quad = 0u, at_q = 0u, at_l = 0u;
    unsigned long long bad = 0ull, first = ~0ull;
    for (int walk = 0; walk < 2; ++walk) {
        for (uint32_t c0 = 0u; c0 < n_cand; c0 += 64u) {
            const uint32_t c = c0 + lane;
            bool live = false, lin = false;
            Cand want;
            if (c < n_cand) {
                Rec r;
                RowGuess g;
                record_prep<0>(seg_pts + 6u * (size_t)(s0 + (c >> 1)), c & 1u, G, r, g);
                if (!g.empty) {
                    want.cut = find_cut(r);
                    live = want.cut.lo <= want.cut.hi;
                    lin = (int32_t)r.flags < 0;
                    want.rec = c4_make_rec40<0>(r, 0u, 0u);
                }
            }
            const unsigned long long mq = __ballot(live && !lin), ml = __ballot(live && lin);
            if (walk == 0) { n_quad += (uint32_t)__popcll(mq); continue; }
            if (live) {
                const uint32_t slot = lin ? n_quad + at_l + (uint32_t)__popcll(ml & below) : at_q + (uint32_t)__popcll(mq & below);
                const Cand got = tab[base + slot];
                uint32_t w[12], v[12];
                __builtin_memcpy(w, &want, 48);
                __builtin_memcpy(v, &got, 48);
                bool same = true;
#pragma unroll
                for (int i = 0; i < 12; ++i) same = same && w[i] == v[i];
                if (!same) { ++bad; first = min(first, ((unsigned long long)gl << 32) | slot); }
            }
            at_q += (uint32_t)__popcll(mq);
            at_l += (uint32_t)__popcll(ml);
        }
    }
    const uint32_t n_live = n_quad + at_l;
    for (uint32_t slot = n_live + lane; slot < n_cand; slot += 64u) {
        const Cand got = tab[base + slot];
        if (!(c4_cand_dead(got) && !(got.cut.lo <= got.cut.hi))) { ++bad; first = min(first, ((unsigned long long)gl << 32) | slot); }
    }
    if (lane == 0u) { glyph_live[gl] = n_live; atomicAdd(&res[0], (unsigned long long)n_live); }
    if (bad) { atomicAdd(&res[1], bad); atomicMin(&res[2], first); }
}

// res: three words, zero-initialised but res[2] all ones; glyph_live: n_glyphs words
void launch_selftest_cand_records(const uint32_t *glyph_seg_start, const int16_t *seg_pts, const uint4 *tab, uint32_t n_glyphs,
                                  unsigned long long *res, uint32_t *glyph_live, hipStream_t stream)
{
    if (n_glyphs == 0) return;
    hipLaunchKernelGGL(selftest_cand_records_kernel, dim3(n_glyphs), dim3(64), 0, stream, glyph_seg_start, seg_pts,
                       reinterpret_cast<const Cand *>(tab), n_glyphs, res, glyph_live);
}

}  // namespace fr

extern "C" int fr_selftest_sqrt_fast(int variant, uint64_t *mismatches, uint32_t *bad_x_bits)
{
    if (!mismatches || variant < 0 || variant > 1) return FR_E_INVALID;
    unsigned long long *d_m = nullptr;
    uint32_t *d_b = nullptr;
    if (hipMalloc(&d_m, 8) != hipSuccess || hipMalloc(&d_b, 8) != hipSuccess) return FR_E_HIP;
    (void)hipMemset(d_m, 0, 8);
    (void)hipMemset(d_b, 0, 8);
    const uint32_t e_lo = 97u, e_hi = 192u;                        // [2^-30, 2^66), as fr_selftest_sqrt
    const dim3 grid((e_hi - e_lo + 1u) * 32u), block(256);
    if (variant == 0) hipLaunchKernelGGL(fr::selftest_sqrt_fast_kernel<0>, grid, block, 0, 0, e_lo, d_m, d_b);
    else hipLaunchKernelGGL(fr::selftest_sqrt_fast_kernel<1>, grid, block, 0, 0, e_lo, d_m, d_b);
    unsigned long long m = 0;
    uint32_t b = 0;
    hipError_t e = hipMemcpy(&m, d_m, 8, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(&b, d_b, 4, hipMemcpyDeviceToHost);
    (void)hipFree(d_m);
    (void)hipFree(d_b);
    if (e != hipSuccess) return FR_E_HIP;
    *mismatches = m;
    if (bad_x_bits) *bad_x_bits = b;
    return FR_OK;
}

extern "C" int fr_selftest_sqrt(uint64_t *mismatches, uint32_t *bad_x_bits)
{
    if (!mismatches) return FR_E_INVALID;
    unsigned long long *d_m = nullptr;
    uint32_t *d_b = nullptr;
    if (hipMalloc(&d_m, 8) != hipSuccess || hipMalloc(&d_b, 8) != hipSuccess) return FR_E_HIP;
    (void)hipMemset(d_m, 0, 8);
    (void)hipMemset(d_b, 0, 8);
    // exponent fields 97 .. 192: [2^-30, 2^66) covers every delta the path can form (and then some)
    const uint32_t e_lo = 97u, e_hi = 192u;
    hipLaunchKernelGGL(fr::selftest_sqrt_kernel, dim3((e_hi - e_lo + 1u) * 32u), dim3(256), 0, 0, e_lo, d_m, d_b);
    // the two special arguments: 0 -> 0, negative -> NaN are checked on the host side of the test
    unsigned long long m = 0;
    uint32_t b = 0;
    hipError_t e = hipMemcpy(&m, d_m, 8, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(&b, d_b, 4, hipMemcpyDeviceToHost);
    (void)hipFree(d_m);
    (void)hipFree(d_b);
    if (e != hipSuccess) return FR_E_HIP;
    *mismatches = m;
    if (bad_x_bits) *bad_x_bits = b;
    return FR_OK;
}

extern "C" int fr_selftest_division(uint32_t d_lo, uint32_t d_hi, uint64_t *mismatches,
                                    uint32_t *bad_divisor, uint32_t *bad_x_bits)
{
    if (!mismatches || d_lo < 1 || d_hi < d_lo || d_hi > (1u << 17)) return FR_E_INVALID;
    unsigned long long *d_m = nullptr;
    uint32_t *d_b = nullptr;
    if (hipMalloc(&d_m, 8) != hipSuccess || hipMalloc(&d_b, 8) != hipSuccess) return FR_E_HIP;
    (void)hipMemset(d_m, 0, 8);
    (void)hipMemset(d_b, 0, 8);
    const uint32_t n_d = d_hi - d_lo + 1;
    for (uint32_t off = 0; off < n_d; off += 4096u) {              // <= 131072 blocks per launch
        const uint32_t n = n_d - off < 4096u ? n_d - off : 4096u;
        hipLaunchKernelGGL(fr::selftest_div_kernel, dim3(n * 32u), dim3(256), 0, 0, d_lo + off, n, d_m, d_b);
    }
    unsigned long long m = 0;
    uint32_t b[2] = {0, 0};
    hipError_t e = hipMemcpy(&m, d_m, 8, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(b, d_b, 8, hipMemcpyDeviceToHost);
    (void)hipFree(d_m);
    (void)hipFree(d_b);
    if (e != hipSuccess) return FR_E_HIP;
    *mismatches = m;
    if (bad_divisor) *bad_divisor = b[0];
    if (bad_x_bits) *bad_x_bits = b[1];
    return FR_OK;
}

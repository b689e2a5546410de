// fr_c4.hpp — what cov4_kernel (fr_cov4.hip, 16 samples per pixel) and win1_kernel (fr_win1.hip, 1 sample per pixel)
// share: the 40-byte root record, the workgroup set-up (records with exact row ranges + cx table).
#pragma once
#include "fr_records.hpp"
#include "fr_wave.hpp"

namespace fr {

#ifndef FR_C4_WAVES
#define FR_C4_WAVES 4
#endif
#ifndef FR_C4_OCC
#define FR_C4_OCC 4
#endif
#ifndef FR_C4_PCAP
#define FR_C4_PCAP 448
#endif
#ifndef FR_C4_OCC_SMALL
#define FR_C4_OCC_SMALL 6
#endif
#ifndef FR_DYN_BANDS
#define FR_DYN_BANDS 1
#endif
#ifndef FR_W1_OCC_SMALL
#define FR_W1_OCC_SMALL 6
#endif
// PCAP: (record, row) pairs laid out per round (a multiple of 64).
enum { C4_WAVES = FR_C4_WAVES, C4_PCAP = FR_C4_PCAP };
// u16 slots per row list: the CAP crossings a row keeps + the dump slot + padding to a multiple of 4 (8-byte rows).
// (36 for CAP = 32; the instances that keep 16 or 8 have shorter rows and leave the LDS to more workgroups)
constexpr uint32_t c4_lstride(int cap) { return (uint32_t)cap + 4u; }
// Waves per SIMD the register allocation is held to.  The instances that keep <= 16 crossings per row with two records
// per lane (glyphs of <= 128 candidate roots: ASCII-like, a real font) need <= 26 KB of LDS per workgroup, so SIX
// workgroups fit a CU if the kernel stays within 80 VGPRs: measured 0.0754 -> 0.0643 ms on configs[3]'s shard (128^2
// cells), 0.343 -> 0.291 ms on 256^2 cells of 32 segments — and nothing at five (an odd number of waves per SIMD: DESIGN.md
// section 4.0).  The instances that keep 32 crossings or more records are bound to four (three) by their LDS.
// (the 1024-record instances: 77 KB of LDS, two workgroups per CU — the register budget of two waves per SIMD)
// (the 512-record instances: 45 - 53 KB of LDS, three workgroups per CU — and a third of the register file each, which the
// second register list of their two-pass bands needs: fr_cov4.hip, SPLIT)
constexpr int c4_occ(int cap, int wlog, int rpl) { return rpl >= 16 ? 2 : (rpl >= 8 ? 3 : ((cap <= 16 && rpl == 2) ? FR_C4_OCC_SMALL : FR_C4_OCC)); }
constexpr int w1_occ(int rpl, int wlog) { return rpl >= 16 ? 2 : ((rpl == 2) ? FR_W1_OCC_SMALL : FR_C4_OCC); }
// 16 bytes of a row list (8-byte aligned): two 8-byte LDS accesses unless the rows are 16-byte aligned
template <uint32_t LSTRIDE>
__device__ __forceinline__ uint4 c4_ld16(const uint16_t *p)
{
    if ((LSTRIDE * 2) % 16 == 0) return *reinterpret_cast<const uint4 *>(p);
    const uint2 a = reinterpret_cast<const uint2 *>(p)[0], b = reinterpret_cast<const uint2 *>(p)[1];
    return make_uint4(a.x, a.y, b.x, b.y);
}
template <uint32_t LSTRIDE>
__device__ __forceinline__ void c4_st16(uint16_t *p, uint4 v)
{
    if ((LSTRIDE * 2) % 16 == 0) { *reinterpret_cast<uint4 *>(p) = v; return; }
    reinterpret_cast<uint2 *>(p)[0] = make_uint2(v.x, v.y);
    reinterpret_cast<uint2 *>(p)[1] = make_uint2(v.z, v.w);
}

// 40-byte root record of the cov4 kernel (LDS only)
struct __attribute__((aligned(8))) Rec40 {
    float a;        // quadratic: p0y - 2 p1y + p2y (:48); linear (a == 0 branch): the divisor p2y - p0y (:51)
    float b;        // quadratic: p0y - p1y;               linear: p0y
    float c1, c2;   // quadratic: p1y^2, p0y p2y (:58);    linear: 0
    float ax, bx, p0x;   // (:53 / :65)
    float rden;     // RN(1 / a)
    float sgn;      // +1 for the t+ root, -1 for t-  (sqrt * +-1 is exact: B - sqrt == B + (-sqrt))
    uint32_t fr;    // ra | re << 12 | cb << 24 | zb << 26 | linear << 31 (ra, re <= 2048): sample rows [ra, re) accept the root;
                    // the crossing's step code is (dy > 0) ? zb : cb   (2: +1, 0: -1; :55, :68)
};

// One slot of a glyph set's candidate table (cand_kernel, fr_prepare.hip): a candidate root's record
// as the set-up would build it — every field depends on the segment's control points and the root alone — with the range
// bits of `fr` clear, and its row cut.  48 bytes, three 16-byte loads.  A glyph's slice [2 seg0, 2 seg0 + 2 nseg) holds its
// live candidates (record_prep does not discard them, and their cut is not empty) in record order — quadratic first,
// linear last, each group in candidate order — and then dead slots: all zero, the empty cut {+inf, -inf}.  A live record
// divides by `a`, so a == 0 in the first 16 bytes marks a dead slot.
struct __attribute__((aligned(16))) Cand {
    Rec40 rec;
    Cut cut;
};
static_assert(sizeof(Cand) == 48, "three 16-byte loads per candidate");
__device__ __forceinline__ bool c4_cand_dead(const Cand &e) { return e.rec.a == 0.0f; }

// select on a wave mask held in SGPRs — the VOP3 form, whose cost does not depend on what wrote the mask
// (a VOP2 v_cndmask reading a VCC that is not fresh costs 3-5 vector instructions: profiles/r02/issue_model3.txt)
__device__ __forceinline__ uint32_t c4_sel(unsigned long long m, uint32_t if_set, uint32_t if_clear)
{
    uint32_t r;
    asm("v_cndmask_b32_e64 %0, %1, %2, %3" : "=v"(r) : "v"(if_clear), "v"(if_set), "s"(m));
    return r;
}
__device__ __forceinline__ float c4_self(unsigned long long m, float if_set, float if_clear)
{
    return __builtin_bit_cast(float, c4_sel(m, __builtin_bit_cast(uint32_t, if_set), __builtin_bit_cast(uint32_t, if_clear)));
}
// 16-byte streaming store of finished pixels (never read again by this kernel): the non-temporal hint keeps them from
// displacing the tables the kernel does re-read in L2
__device__ __forceinline__ void c4_store16(void *dst, uint4 v)
{
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    typedef u32x4 u32x4_u __attribute__((aligned(4)));
    u32x4 w = {v.x, v.y, v.z, v.w};
    __builtin_nontemporal_store(w, reinterpret_cast<u32x4_u *>(dst));
}

// a settled candidate as the kernels keep it (40 bytes): row range [ra, re) in the low bits of `fr`.
// FILL = 1 (FR_FILL_CONSISTENT): zb == cb == the piece's step code (flags & 2, fr_records.hpp), whatever dy says.
template <int FILL = 0>
__device__ __forceinline__ Rec40 c4_make_rec40(const Rec &r, uint32_t ra, uint32_t re)
{
    Rec40 m;
    const bool lin = (int32_t)r.flags < 0;
    m.a = lin ? r.c1 : r.a;
    m.b = r.b; m.c1 = lin ? 0.0f : r.c1; m.c2 = r.c2;
    m.ax = r.ax; m.bx = r.bx; m.p0x = r.p0x; m.rden = r.rden;
    m.sgn = r.sqsign ? -1.0f : 1.0f;
    const uint32_t cb = (lin || FILL) ? (r.flags & 2u) : 2u, zb = (lin || FILL) ? cb : 0u;
    m.fr = ra | (re << 12) | (cb << 24) | (zb << 26) | (lin ? 0x80000000u : 0u);
    return m;
}

// The strip's exact sample abscissae cx(j) = (f32(min_x + x) + off(i)) / scale (:26) into s_cxp[1 + j], thread `tid` of STEP.
// Two loops, chosen once by the workgroup-uniform `sdiv.pow2` — written as one loop the compiler computes the quotient
// both ways for every entry and selects.
template <int N, uint32_t NCOL, uint32_t STEP>
__device__ __forceinline__ void c4_fill_cx(float *s_cxp, uint32_t tid, int32_t min_xs, int phase, const ScaleDiv &sdiv)
{
    auto num = [&](uint32_t j) { return (float)(min_xs + (int32_t)(j / (uint32_t)N)) + sub_off((int)(j % (uint32_t)N), N, phase); };
    if (sdiv.pow2) {
        for (uint32_t j = tid; j < NCOL; j += STEP) s_cxp[1u + j] = num(j) * sdiv.inv;
    } else {
        for (uint32_t j = tid; j < NCOL; j += STEP) s_cxp[1u + j] = num(j) / sdiv.scale;
    }
}

// the row cut (fr_records.hpp) of candidate c = 2 segment + root of the glyph whose first segment is seg0: one 8-byte
// load beside the candidate's control points, not after them
__device__ __forceinline__ Cut c4_load_cut(const RenderArgs &A, uint32_t seg0, uint32_t c)
{
    const float2 q = reinterpret_cast<const float2 *>(A.seg_cut)[2u * (size_t)seg0 + c];
    Cut k;
    k.lo = q.x; k.hi = q.y;
    return k;
}

// Slot c of the glyph's slice of the candidate table, and the row range guessed from its cut: the first row at or below
// `hi` and the first row below `lo`, where the class changes in exact arithmetic.  As record_prep's, the guess only decides
// how many rows record_settle looks at.  A dead slot has the empty cut, which misses every cell.
__device__ __forceinline__ Cand c4_load_cand(const RenderArgs &A, uint32_t seg0, uint32_t c)
{
    return reinterpret_cast<const Cand *>(A.seg_cand)[2u * (size_t)seg0 + c];
}
__device__ __forceinline__ void c4_cand_guess(const Cut &k, const RowGeom &G, RowGuess &g)
{
    g.empty = cut_misses(k, row_span(G));
    g.ra = 1u; g.re = 0u;
    if (!g.empty) {
        const float top = (float)G.rows;
        g.ra = (uint32_t)fminf(fmaxf(__builtin_ceilf(G.row_of(k.hi)), 0.0f), top);
        g.re = (uint32_t)fminf(fmaxf(__builtin_floorf(G.row_of(k.lo)) + 1.0f, 0.0f), top);
    }
}
// the settled candidate: the table's record with its row range in the low bits of `fr`
__device__ __forceinline__ Rec40 c4_cand_rec40(const Rec40 &m, uint32_t ra, uint32_t re)
{
    Rec40 o = m;
    o.fr |= ra | (re << 12);
    return o;
}

// Set-up for glyphs of <= 32 segments (<= 64 candidate roots: one per lane of ONE wave — ASCII-like glyphs), four
// waves.  Settling a candidate's row range costs four evaluations of the reference's acceptance at the rows around
// the two guessed ends; with the plain set-up wave 0 would do all of it while waves 1 - 3 (and the SIMDs they sit
// on) wait.  Here every wave prepares the same 64 candidates and looks at ONE of the four rows (wave 0: ra - 1,
// 1: ra, 2: re - 1, 3: re); wave 0 takes the guess when the four classes confirm it — exactly the condition under
// which record_settle's walks would not move — and walks as before otherwise.  Same records, same order.
// CUT = 1 (every set-up below): the class of a row is read off the candidate's row cut (A.seg_cut is not null, FILL = 0)
// CUT = 2: the same, and lane c takes slot c of the glyph's candidate table (A.seg_cand is not null, FILL = 0) instead of
// building candidate c: the slots are in record order already, so one ballot places the records, and a wave whose slots
// are all dead has nothing to do between the barriers
template <uint32_t RCAP, int N, uint32_t NCOL, int FILL, int CUT>
__device__ __forceinline__ uint32_t c4_setup_small(const RenderArgs &A, const Job &job, uint32_t seg0, uint32_t nseg, uint32_t x0s,
                                                   int phase, float *s_cxp, Rec40 *s_rec, uint32_t *s_wcnt, uint32_t *s_tmp, const float *cyt = nullptr)
{
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t Hs = job.h * (uint32_t)N;
    const ScaleDiv sdiv = scale_div(job.scale);         // (a multiply when scale is a power of two: fr_device.hpp)
    RowGeom geo;
    geo.max_y = job.max_y; geo.set_scale(sdiv); geo.rows = Hs; geo.n = N; geo.phase = phase; geo.cyt = cyt;
    const bool have = lane < 2u * nseg;
    Rec r;
    RowGuess g;
    Piece pc;
    g.empty = true; g.ra = 1u; g.re = 0u;
    uint32_t cls = 3u;                                  // 3: no such row / not asked — the condition it stands for holds
    Cut k;
    k.lo = k.hi = 0.0f;
    Rec40 tab;                                          // CUT = 2: the table's record of slot `lane`
    tab.fr = 0u;
    if (have) {
        if constexpr (CUT == 2) {
            const Cand e = c4_load_cand(A, seg0, lane);
            tab = e.rec; k = e.cut;
            c4_cand_guess(k, geo, g);
        } else {
            bool drop = false;
            if constexpr (CUT != 0) { k = c4_load_cut(A, seg0, lane); drop = cut_misses(k, row_span(geo)); }
            record_prep<FILL>(A.seg_pts + 6u * (size_t)(seg0 + (lane >> 1)), lane & 1u, geo, r, g, &pc, drop);
        }
        if (!g.empty) {
            const uint32_t row = (wave == 0u) ? g.ra - 1u : (wave == 1u) ? g.ra : (wave == 2u) ? g.re - 1u : g.re;   // (ra - 1 wraps past the cell at ra = 0)
            if (row < Hs && (wave != 2u || g.re > g.ra)) cls = (uint32_t)row_class<FILL, CUT>(r, pc, geo.cy(row), &k);
        }
    }
    s_tmp[tid] = cls;
    // exact sample abscissae of this strip: cx(j) = (f32(min_x + x) + off(i)) / scale   (:26)
    const int32_t min_xs = job.min_x + (int32_t)x0s;
    c4_fill_cx<N, NCOL, 256u>(s_cxp, tid, min_xs, phase, sdiv);
    if (tid == 2) s_cxp[0] = -__builtin_inff();
    if (tid == 3) s_cxp[1u + NCOL] = __builtin_inff();
    __syncthreads();
    if (wave == 0u) {
        Rec40 mine;
        mine.fr = 0u;
        bool live = false;
        if (have) {
            uint32_t ra = g.ra, re = g.re;
            if (!g.empty) {
                const uint32_t c0 = s_tmp[lane], c1 = s_tmp[64u + lane], c2 = s_tmp[128u + lane], c3 = s_tmp[192u + lane];
                // record_settle would leave (ra, re) alone iff: the row above ra is rejected from above (class 2), ra is
                // not (class <= 1), re >= ra, the row before re is accepted (class >= 1), re is below the set (class 0)
                const bool ok = (c0 >= 2u) && (c1 <= 1u || c1 == 3u) && re >= ra && (c2 >= 1u) && (c3 == 0u || c3 == 3u);
                if (!ok) record_settle<FILL, CUT>(r, geo, ra, re, &pc, &k);
            }
            live = ra < re;
            if constexpr (CUT == 2) mine = c4_cand_rec40(tab, ra, re);
            else mine = c4_make_rec40<FILL>(r, ra, re);
        }
        // quadratic records first, linear ones last (as c4_setup); the candidate table's slots are in that order already
        const bool linr = CUT != 2 && live && (int32_t)mine.fr < 0;
        const unsigned long long lm = __ballot(live && !linr), ll = (CUT == 2) ? 0ull : __ballot(linr), below = (1ull << lane) - 1ull;
        const uint32_t n_quad = (uint32_t)__popcll(lm);
        uint32_t pos = RCAP;
        if ((lm >> lane) & 1ull) pos = (uint32_t)__popcll(lm & below);
        if ((ll >> lane) & 1ull) pos = n_quad + (uint32_t)__popcll(ll & below);
        if (pos < RCAP) s_rec[pos] = mine;
        if (lane == 0u) s_wcnt[0] = min(n_quad + (uint32_t)__popcll(ll), RCAP);
    }
    __syncthreads();
    return s_wcnt[0];
}

// The same for 33 .. 64 segments (<= 128 candidate roots: one per lane of waves 0 and 1).  Thread c + 128 h looks at the
// rows around the upper end (h = 0: ra - 1 and ra) or the lower end (h = 1: re - 1 and re) of candidate c; the owners
// (h = 0) take the guess when all four classes confirm it and walk otherwise.
template <uint32_t RCAP, int N, uint32_t NCOL, int FILL, int CUT>
__device__ __forceinline__ uint32_t c4_setup_mid(const RenderArgs &A, const Job &job, uint32_t seg0, uint32_t nseg, uint32_t x0s,
                                                 int phase, float *s_cxp, Rec40 *s_rec, uint32_t *s_wcnt, uint32_t *s_tmp, const float *cyt = nullptr)
{
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t c = tid & 127u, h = tid >> 7;
    const uint32_t Hs = job.h * (uint32_t)N;
    const ScaleDiv sdiv = scale_div(job.scale);
    RowGeom geo;
    geo.max_y = job.max_y; geo.set_scale(sdiv); geo.rows = Hs; geo.n = N; geo.phase = phase; geo.cyt = cyt;
    const bool have = c < 2u * nseg;
    Rec r;
    RowGuess g;
    Piece pc;
    g.empty = true; g.ra = 1u; g.re = 0u;
    uint32_t cls0 = 3u, cls1 = 3u;                      // 3: no such row / not asked
    Cut k;
    k.lo = k.hi = 0.0f;
    Rec40 tab;                                          // CUT = 2: the table's record of slot c
    tab.fr = 0u;
    if (have) {
        if constexpr (CUT == 2) {
            const Cand e = c4_load_cand(A, seg0, c);
            tab = e.rec; k = e.cut;
            c4_cand_guess(k, geo, g);
        } else {
            bool drop = false;
            if constexpr (CUT != 0) { k = c4_load_cut(A, seg0, c); drop = cut_misses(k, row_span(geo)); }
            record_prep<FILL>(A.seg_pts + 6u * (size_t)(seg0 + (c >> 1)), c & 1u, geo, r, g, &pc, drop);
        }
        if (!g.empty) {
            const uint32_t end = h ? g.re : g.ra;       // rows end - 1 and end
            if (end - 1u < Hs && (h == 0u || g.re > g.ra)) cls0 = (uint32_t)row_class<FILL, CUT>(r, pc, geo.cy(end - 1u), &k);
            if (end < Hs) cls1 = (uint32_t)row_class<FILL, CUT>(r, pc, geo.cy(end), &k);
        }
    }
    s_tmp[tid] = cls0 | (cls1 << 8);
    const int32_t min_xs = job.min_x + (int32_t)x0s;
    c4_fill_cx<N, NCOL, 256u>(s_cxp, tid, min_xs, phase, sdiv);
    if (tid == 2) s_cxp[0] = -__builtin_inff();
    if (tid == 3) s_cxp[1u + NCOL] = __builtin_inff();
    __syncthreads();
    Rec40 mine;
    mine.fr = 0u;
    bool live = false;
    if (h == 0u && have) {
        uint32_t ra = g.ra, re = g.re;
        if (!g.empty) {
            const uint32_t up = s_tmp[c], dn = s_tmp[128u + c];
            const uint32_t c0 = up & 0xffu, c1 = up >> 8, c2 = dn & 0xffu, c3 = dn >> 8;
            const bool ok = (c0 >= 2u) && (c1 <= 1u || c1 == 3u) && re >= ra && (c2 >= 1u) && (c3 == 0u || c3 == 3u);
            if (!ok) record_settle<FILL, CUT>(r, geo, ra, re, &pc, &k);
        }
        live = ra < re;
        if constexpr (CUT == 2) mine = c4_cand_rec40(tab, ra, re);
        else mine = c4_make_rec40<FILL>(r, ra, re);
    }
    // quadratic records first, linear ones last (as c4_setup): waves 0 and 1 hold them; the candidate table's slots are in
    // that order already
    const bool linr = CUT != 2 && live && (int32_t)mine.fr < 0;
    const unsigned long long lm = __ballot(live && !linr), ll = (CUT == 2) ? 0ull : __ballot(linr), below = (1ull << lane) - 1ull;
    if (lane == 0u && wave < 2u) { s_wcnt[wave] = (uint32_t)__popcll(lm); s_wcnt[2u + wave] = (uint32_t)__popcll(ll); }
    __syncthreads();
    const uint32_t q0 = s_wcnt[0], q1 = s_wcnt[1], l0 = s_wcnt[2], l1 = s_wcnt[3];
    const uint32_t n_quad = q0 + q1;
    uint32_t pos = RCAP;
    if ((lm >> lane) & 1ull) pos = (wave ? q0 : 0u) + (uint32_t)__popcll(lm & below);
    if ((ll >> lane) & 1ull) pos = n_quad + (wave ? l0 : 0u) + (uint32_t)__popcll(ll & below);
    if (wave < 2u && pos < RCAP) s_rec[pos] = mine;
    __syncthreads();
    return min(n_quad + l0 + l1, RCAP);
}

// Set-up of a workgroup of NW waves for one cell strip: candidate roots tid, tid + 64 NW, ... (<= 256 segments; <= 384 where RCAP = 512) with the
// exact range of this cell's sample rows that accept each (fr_records.hpp), compacted into s_rec (<= RCAP kept), and
// the padded table of the strip's exact sample abscissae.  Two workgroup barriers.  -> number of records.
// N: samples per pixel axis (4: cov4_kernel, 1: win1_kernel); NCOL: sample columns of the strip.
template <uint32_t NW, uint32_t RCAP, int N, uint32_t NCOL, int FILL, int CUT>
__device__ __forceinline__ uint32_t c4_setup_with(const RenderArgs &A, const Job &job, uint32_t seg0, uint32_t nseg, uint32_t x0s,
                                                  int phase, float *s_cxp, Rec40 *s_rec, uint32_t *s_wcnt, uint32_t *s_tmp, const float *cyt)
{
    if (NW == 4u && 2u * nseg <= 64u)                                        // (workgroup-uniform; s_tmp: 1 KB, free until the bands start)
        return c4_setup_small<RCAP, N, NCOL, FILL, CUT>(A, job, seg0, nseg, x0s, phase, s_cxp, s_rec, s_wcnt, s_tmp, cyt);
    if (NW == 4u && 2u * nseg <= 128u)
        return c4_setup_mid<RCAP, N, NCOL, FILL, CUT>(A, job, seg0, nseg, x0s, phase, s_cxp, s_rec, s_wcnt, s_tmp, cyt);
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t Hs = job.h * (uint32_t)N;
    const ScaleDiv sdiv = scale_div(job.scale);
    // candidates per thread: <= 768 segments where 1024 records are kept, <= 384 where 512, else <= 256
    constexpr uint32_t CPT = (RCAP >= 1024u ? 1536u : (RCAP >= 512u ? 768u : 512u)) / (64u * NW);
    s_wcnt = s_tmp;                                                          // (2 CPT NW counters: the scratch block has the room)
    Rec40 mine[CPT];
    unsigned long long lm[CPT], ll[CPT];
#pragma unroll
    for (uint32_t it = 0; it < CPT; ++it) {
        const uint32_t c = tid + it * 64u * NW;
        bool live = false;
        lm[it] = 0ull; ll[it] = 0ull;
        mine[it].fr = 0u;
        if (it > 0 && it * 64u * NW >= 2u * nseg) continue;                 // workgroup-uniform: no second candidate
        if constexpr (CUT == 2) {
            if (c < 2u * nseg) {
                const Cand e = c4_load_cand(A, seg0, c);
                // (a wave whose slots are all dead — the fourth of a 128-segment glyph, with at most 192 live candidates —
                // skips the block: the compiler branches on an empty execution mask)
                if (!c4_cand_dead(e)) {
                    RowGeom geo;
                    geo.max_y = job.max_y; geo.set_scale(sdiv); geo.rows = Hs; geo.n = N; geo.phase = phase; geo.cyt = cyt;
                    RowGuess g;
                    c4_cand_guess(e.cut, geo, g);
                    uint32_t ra = g.ra, re = g.re;
                    Rec none;                                                    // (record_settle reads the cut alone)
                    if (!g.empty) record_settle<0, 1>(none, geo, ra, re, nullptr, &e.cut);
                    live = ra < re;
                    mine[it] = c4_cand_rec40(e.rec, ra, re);
                }
            }
            // the slots are in record order: one ballot
            lm[it] = __ballot(live);
            if (lane == 0) s_wcnt[it * NW + wave] = (uint32_t)__popcll(lm[it]);
            continue;
        }
        if (c < 2u * nseg) {
            Rec r;
            RowGeom geo;
            geo.max_y = job.max_y; geo.set_scale(sdiv); geo.rows = Hs; geo.n = N; geo.phase = phase; geo.cyt = cyt;
            if constexpr (CUT != 0) {
                const Cut k = c4_load_cut(A, seg0, c);
                const RowSpan span = row_span(geo);
                build_record_rows<FILL, CUT>(A.seg_pts + 6u * (size_t)(seg0 + (c >> 1)), c & 1u, geo, r, &k, &span);
            } else {
                build_record_rows<FILL>(A.seg_pts + 6u * (size_t)(seg0 + (c >> 1)), c & 1u, geo, r);
            }
            const uint32_t ra = __builtin_bit_cast(uint32_t, r.lo), re = __builtin_bit_cast(uint32_t, r.hi);
            live = ra < re;
            mine[it] = c4_make_rec40<FILL>(r, ra, re);
        }
        // quadratic records first, linear ones (the a == 0 branch) last: the pair sequence follows the record order,
        // so an evaluation trip is almost always all-quadratic or all-linear and takes a body without the other's work
        const bool linr = live && (int32_t)mine[it].fr < 0;
        lm[it] = __ballot(live && !linr);
        ll[it] = __ballot(linr);
        if (lane == 0) { s_wcnt[it * NW + wave] = (uint32_t)__popcll(lm[it]); s_wcnt[CPT * NW + it * NW + wave] = (uint32_t)__popcll(ll[it]); }
    }
    // exact sample abscissae of this strip: cx(j) = (f32(min_x + x) + off(i)) / scale   (:26)
    const int32_t min_xs = job.min_x + (int32_t)x0s;
    c4_fill_cx<N, NCOL, 64u * NW>(s_cxp, tid, min_xs, phase, sdiv);
    if (tid == 2) s_cxp[0] = -__builtin_inff();
    if (tid == 3) s_cxp[1u + NCOL] = __builtin_inff();
    __syncthreads();
    uint32_t rec_cnt = 0;
    {
        uint32_t base_q[CPT], base_l[CPT], n_quad = 0;
#pragma unroll
        for (uint32_t it = 0; it < CPT; ++it) base_q[it] = base_l[it] = 0;
#pragma unroll
        for (uint32_t q = 0; q < CPT * NW; ++q) {
            if (q >= NW && q / NW * 64u * NW >= 2u * nseg) continue;        // (never written)
            const uint32_t cq = s_wcnt[q], cl = (CUT == 2) ? 0u : s_wcnt[CPT * NW + q];
#pragma unroll
            for (uint32_t it = 0; it < CPT; ++it) {
                base_q[it] += (q < it * NW + wave) ? cq : 0u;
                base_l[it] += (q < it * NW + wave) ? cl : 0u;
            }
            n_quad += cq;
            rec_cnt += cq + cl;
        }
#pragma unroll
        for (uint32_t it = 0; it < CPT; ++it) {
            const unsigned long long below = (1ull << lane) - 1ull;
            uint32_t pos = RCAP;
            if ((lm[it] >> lane) & 1ull) pos = base_q[it] + (uint32_t)__popcll(lm[it] & below);
            if ((ll[it] >> lane) & 1ull) pos = n_quad + base_l[it] + (uint32_t)__popcll(ll[it] & below);
            if (pos < RCAP) s_rec[pos] = mine[it];                          // (the plan only sends glyphs with <= RCAP possible records)
        }
    }
    rec_cnt = min(rec_cnt, RCAP);
    __syncthreads();
    return rec_cnt;
}

// the set-up from the glyph set's candidate table where the launch has it (A.seg_cand), else with its row cuts where the
// launch has them (A.seg_cut), else without: the same for the whole grid
template <uint32_t NW, uint32_t RCAP, int N, uint32_t NCOL, int FILL = 0>
__device__ __forceinline__ uint32_t c4_setup(const RenderArgs &A, const Job &job, uint32_t seg0, uint32_t nseg, uint32_t x0s,
                                             int phase, float *s_cxp, Rec40 *s_rec, uint32_t *s_wcnt, uint32_t *s_tmp, const float *cyt = nullptr)
{
    // (FR_C4_ROW_CUTS: listing builds that hold one of the three paths alone — tools/trip_cost.py prices each; never shipped)
#if !defined(FR_C4_ROW_CUTS) || FR_C4_ROW_CUTS == 2
    if constexpr (FILL == 0) {
#ifndef FR_C4_ROW_CUTS
        if (A.seg_cand)
#endif
            return c4_setup_with<NW, RCAP, N, NCOL, 0, 2>(A, job, seg0, nseg, x0s, phase, s_cxp, s_rec, s_wcnt, s_tmp, cyt);
    }
#endif
#if !defined(FR_C4_ROW_CUTS) || FR_C4_ROW_CUTS == 1
    if constexpr (FILL == 0) {
#ifndef FR_C4_ROW_CUTS
        if (A.seg_cut)
#endif
            return c4_setup_with<NW, RCAP, N, NCOL, 0, 1>(A, job, seg0, nseg, x0s, phase, s_cxp, s_rec, s_wcnt, s_tmp, cyt);
    }
#endif
    return c4_setup_with<NW, RCAP, N, NCOL, FILL, 0>(A, job, seg0, nseg, x0s, phase, s_cxp, s_rec, s_wcnt, s_tmp, cyt);
}

}  // namespace fr

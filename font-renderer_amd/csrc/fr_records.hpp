// fr_records.hpp — root records with GUARANTEED acceptance brackets (shared by the stand-alone
// prepare_kernel and by the render kernel, which builds the records of its glyph in LDS).
//
// Why a bracket is sound.  For one root of one segment the reference decides "accept" from
// (render_glyph.zig:58-64)
//        delta = fl(fl(fl(cy*a) + c1) - c2);   reject if delta < 0
//        t     = fl(fl(B +/- sqrt(delta)) / a); reject if t < 0 or t >= 1
// with a, B, c1, c2 constants of the segment.  Every step is a correctly rounded IEEE
// operation with one varying operand, hence a monotone function of it; so delta(cy) is
// monotone (direction = sign a), sqrt is non-decreasing, and t+(cy) is non-decreasing /
// t-(cy) non-increasing for either sign of a.  The three rejection tests are therefore each a
// one-sided cut of the cy axis: classify() below is a monotone step function 0 -> 1 -> 2
// ("below the accepted set", "accepted", "above it") over the ordered binary32 values.
// Consequently ONE probe with class 0 proves that every smaller cy is rejected, and one probe
// with class 2 proves the same for every larger cy.  We probe the three heights where the
// cuts sit in exact arithmetic (t = 0 at p0y, t = 1 at p2y, delta = 0 at the vertex) and a few
// rounding-plateau widths either side of them, evaluating the reference's own expression, and
// keep  lo = just above the highest class-0 probe,  hi = just below the lowest class-2 probe.
// [lo, hi] CONTAINS the accepted set (exactly, not approximately); the render kernel culls
// with it and still applies the reference's own three tests to whatever survives, so the
// bracket only ever saves work.  The same holds for the a == 0 branch (:51-52).
#pragma once
#include "fr_device.hpp"

namespace fr {

// 0 = cy lies below the accepted interval, 1 = accepted, 2 = above
__device__ __forceinline__ int classify(const Rec &r, float cy)
{
    if (r.flags & REC_LINEAR) {
        float t = rec_t_lin(r, cy);
        bool up = r.c1 > 0.0f;                         // den > 0: t non-decreasing in cy
        if (t < 0.0f) return up ? 0 : 2;               // :52
        if (t >= 1.0f) return up ? 2 : 0;
        return 1;
    }
    float delta = cy * r.a + r.c1 - r.c2;              // :58
    if (delta < 0.0f) return (r.a > 0.0f) ? 0 : 2;     // :59
    float t = rec_t_quad(r, cy);
    bool neg = (r.flags & REC_NEG_ROOT) != 0;          // t- is non-increasing in cy
    if (t < 0.0f) return neg ? 2 : 0;                  // :64
    if (t >= 1.0f) return neg ? 0 : 2;
    return 1;
}

// Smallest key k in [L, H] such that class(k) >= T, given the invariant
//   every key <  L has class <  T,   every key >= H has class >= T      (class is monotone).
// Only used when the cheap probes leave a side unbounded (rare): exponential, then bisection.
__device__ __noinline__ uint32_t first_at_least(float ra, float rb, float rc1, float rc2, uint32_t rflags, int T, uint32_t L, uint32_t H)
{
    // by value: passing the record by reference to a non-inlined function would force it into scratch
    Rec r;
    r.a = ra; r.b = rb; r.c1 = rc1; r.c2 = rc2; r.flags = rflags;
    uint32_t step = 1u;
    while (step < (1u << 30) && H - L > 2u * step) {
        const uint32_t pl = L + step - 1u;
        if (classify(r, key2f(pl)) >= T) { H = pl; break; }
        L = pl + 1u;
        const uint32_t ph = H - step;
        if (classify(r, key2f(ph)) < T) { L = ph + 1u; break; }
        H = ph;
        step <<= 1;
    }
    while (L < H) {
        const uint32_t mid = L + ((H - L) >> 1);
        if (classify(r, key2f(mid)) >= T) H = mid; else L = mid + 1u;
    }
    return L;
}

__device__ inline bool accept_bracket(const Rec &r, float p0y, float p2y, float &lo, float &hi)
{
    const uint32_t kmin = f2key(-3.402823466e+38f), kmax = f2key(3.402823466e+38f);
    // LB: every key < LB is class 0.  HB: every key >= HB is class 2.
    uint32_t LB = kmin, HB = kmax + 1u;
    bool seen1 = false;
    auto probe = [&](float c) {
        if (!(c >= -3.402823466e+38f && c <= 3.402823466e+38f)) return;      // hints only
        const uint32_t k = f2key(c);
        const int cl = classify(r, c);
        if (cl == 0) { if (k + 1u > LB) LB = k + 1u; }
        else if (cl == 2) { if (k < HB) HB = k; }
        else seen1 = true;
    };
    // width of one rounding plateau of cy*a + c1 near the glyph: ulp(max|c1|,|c2|) / |a|
    float w = 0.0f;
    float vert = 0.0f;
    const bool quad = !(r.flags & REC_LINEAR);
    if (quad) {
        vert = p0y - (r.b * r.b) / r.a;                                       // vertex: y(B/a)
        const float big = fmaxf(fmaxf(fabsf(r.c1), fabsf(r.c2)), 1.0f);
        w = (big * 1.1920929e-07f) / fabsf(r.a);                              // ~ulp(big)/|a|
    }
    auto probe3 = [&](float c) {
        const float d = fmaxf(4.0f * w, fabsf(c) * 4.76837158e-07f);          // >= 4 plateaus, >= 4 ulp
        probe(c - d);
        probe(c);
        probe(c + d);
    };
    probe3(p0y);                                     // (no array, no dynamic index: stays in registers)
    probe3(p2y);
    if (quad) probe3(vert);
    if (LB >= HB) return false;                          // class 0 up to LB-1, class 2 from HB: never accepted
    // a side the probes did not bound (no class-0 / class-2 probe at all): settle it exactly
    if (LB == kmin) LB = first_at_least(r.a, r.b, r.c1, r.c2, r.flags, 1, kmin, HB);
    if (HB == kmax + 1u) HB = first_at_least(r.a, r.b, r.c1, r.c2, r.flags, 2, LB, kmax + 1u);
    if (LB >= HB) return false;
    (void)seen1;
    lo = key2f(LB);
    hi = key2f(HB - 1u);
    return true;
}


// Candidate root `root` (0: t+, or the single root of an a == 0 segment; 1: t-) of the segment
// whose three control points are p[0..5] (i16 x,y pairs).  Returns false when the root does not
// exist or its bracket is provably empty.
__device__ inline bool build_record(const int16_t *p, uint32_t root, Rec &r)
{
    // i16 -> f32 (render_glyph.zig:43-45)
    const float p0x = (float)p[0], p0y = (float)p[1];
    const float p1x = (float)p[2], p1y = (float)p[3];
    const float p2x = (float)p[4], p2y = (float)p[5];
    const float a = p0y - 2 * p1y + p2y;                 // :48
    r.ax = p0x - 2 * p1x + p2x;                          // :53/:65
    r.bx = 2 * (p1x - p0x);
    r.p0x = p0x;
    r.sqsign = root ? 0x80000000u : 0u;
    if (a == 0.0f) {                                     // :49
        if (root != 0u || p2y == p0y) return false;      // :50
        r.a = 0.0f; r.b = p0y; r.c1 = p2y - p0y; r.c2 = 0.0f;
        r.rden = 1.0f / r.c1;
        r.flags = REC_LINEAR | ((p0y < p2y) ? REC_LIN_MINUS : REC_LIN_PLUS);   // :55
    } else {
        r.a = a; r.b = p0y - p1y; r.c1 = p1y * p1y; r.c2 = p0y * p2y;    // :58, :60
        r.rden = 1.0f / a;
        r.flags = root ? REC_NEG_ROOT : 0u;
    }
    float lo, hi;
    if (!accept_bracket(r, p0y, p2y, lo, hi)) return false;
    r.lo = lo; r.hi = hi;
    return true;
}

// ---------------------------------------------------------------------------------------------
// Row form of the same bracket, used by the render kernel's in-LDS record build.  A cell's sample
// rows have ray heights cy(r) = (f32(max_y - y) - off) / scale (render_glyph.zig:27), non-increasing
// in r, so by the monotonicity argued above the class of row r is NON-INCREASING in r (2 = above
// the accepted set, 1 = accepted, 0 = below) and the accepted rows are ONE half-open range
//        [ra, re),   ra = min{ r : class(r) <= 1 },   re = min{ r >= ra : class(r) == 0 }.
// Both ends are settled by evaluating the reference's own expression at the rows either side of a
// guess and walking while the class says so — the guess (where t = 0, t = 1 and delta = 0 sit in
// exact arithmetic) only decides how many rows are looked at, never the result.  Two candidates
// are discarded without a probe, by a bound that holds for the rounded values too:
//   * the root on the far side of a vertex at t_v = B/a >= 1 is >= fl(B/a) >= 1  (always rejected, :64)
//   * the root on the near side of a vertex at t_v < 0 is <= fl(B/a) < 0          (always rejected, :64)
// (B +/- sqrt(delta) is >= / <= B after rounding because B is representable, and a correctly
// rounded division by a is monotone; |B/a| >= 2^-17 cannot round to zero.)
struct RowGeom {
    int32_t max_y;
    float scale;
    uint32_t rows;       // sample rows of the cell (h * N)
    int n, phase;
    const float *cyt = nullptr;   // optional: the ray heights of all the cell's rows, computed once by this very expression
    float inv = 1.0f;             // scale = +-2^k inside the proven range (ScaleDiv, fr_device.hpp): 1 / scale, and the
    bool pow2 = false;            // division below is this multiply — the same bits.  Left unset: always the division.
    __device__ __forceinline__ void set_scale(const ScaleDiv &d) { scale = d.scale; inv = d.inv; pow2 = d.pow2; }
    __device__ __forceinline__ float cy(uint32_t r) const
    {
        if (cyt) return cyt[r];
        const float num = (float)(max_y - (int32_t)(r / (uint32_t)n)) - sub_off((int)(r % (uint32_t)n), n, phase);
        if (pow2) return num * inv;
        return num / scale;
    }
    // fractional row index at which the ray height equals c (rows r >= x lie at or below c)
    __device__ __forceinline__ float row_of(float c) const
    {
        return ((float)max_y - c * scale) * (float)n - (phase ? 0.5f : 0.0f);
    }
};

// branch-free class of ray height cy for either kind of record; t by div_by_int (== IEEE `/`, fr_device.hpp)
__device__ __forceinline__ int classify_row(const Rec &r, float cy)
{
    const bool lin = (r.flags & REC_LINEAR) != 0;
    const float delta = cy * r.a + r.c1 - r.c2;                                  // :58
    const float sq = sqrt_rn(delta);
    const float num = lin ? (cy - r.b) : ((r.flags & REC_NEG_ROOT) ? (r.b - sq) : (r.b + sq));   // :51 / :60-61
    const float t = div_by_int(num, lin ? r.c1 : r.a, r.rden);
    // t falls with cy for the t- root and for a descending line
    const bool falls = lin ? !(r.c1 > 0.0f) : ((r.flags & REC_NEG_ROOT) != 0);
    int cl = 1;
    if (t >= 1.0f) cl = falls ? 0 : 2;                                           // :52 / :64
    if (t < 0.0f) cl = falls ? 2 : 0;
    if (!lin && delta < 0.0f) cl = (r.a > 0.0f) ? 0 : 2;                         // :59
    return cl;
}

// ---------------------------------------------------------------------------------------------
// FR_FILL_CONSISTENT (include/fr_raster.h): the same sample points, a different crossing rule.
// Every record (t+ / t- root, or the a == 0 root) is one y-monotone PIECE of its segment — the t+ root is the half
// that rises along t, the t- root the half that falls, the a == 0 root the whole line — and a piece with end heights
// ylo < yhi is crossed by the ray at height cy iff  ylo <= cy < yhi  (exact; a piece of zero height is never
// crossed), with step -1 if it rises, +1 if it falls: the step code is (flags & 2) for every record (REC_NEG_ROOT ==
// REC_LIN_PLUS == 2).  The end heights are the integers p0y, p2y and the vertex height y_v = p0y - b^2 / a; the vertex
// test  cy >= y_v  <=>  a (cy - y_v) = a cy + (b^2 - a p0y) has the sign of a (or is 0)  is one f64 FMA of exact
// operands (|a| <= 2^17, cy has 24 significant bits, b^2 - a p0y an integer below 2^34): its rounded result has the
// sign of the exact one.  A pure interval test, so the class is monotone in cy as record_settle needs.
struct Piece {
    float ylo, yhi;      // end heights: exact integers, except the vertex end (vend), where it is an estimate (guess only)
    float a;             // p0y - 2 p1y + p2y
    double cv;           // b^2 - a p0y, exact
    uint32_t vend;       // 0: both ends are on-curve points, 1: the low end is the vertex, 2: the high end is
};
__device__ __forceinline__ bool fill_at_or_above_vertex(const Piece &pc, float cy)
{
    const double d = __builtin_fma((double)pc.a, (double)cy, pc.cv);
    return pc.a > 0.0f ? d >= 0.0 : d <= 0.0;
}
// 0 = cy below the piece, 1 = crossed, 2 = at or above its top
__device__ __forceinline__ int classify_fill(const Piece &pc, float cy)
{
    const bool above = (pc.vend == 2u) ? fill_at_or_above_vertex(pc, cy) : (cy >= pc.yhi);
    const bool below = (pc.vend == 1u) ? !fill_at_or_above_vertex(pc, cy) : (cy < pc.ylo);
    return above ? 2 : (below ? 0 : 1);
}
// ---------------------------------------------------------------------------------------------
// Row cuts.  classify_row is a monotone step function 0 -> 1 -> 2 of cy (the header of this
// file), so a candidate has two keys K1 <= K2 with class 0 below K1, 1 in [K1, K2) and 2 from K2 on.  They depend on the
// segment's control points and the root only — not on cell, scale, sample grid or phase — and cut_kernel (fr_prepare.hip)
// finds them once per glyph set by bisection with classify_row itself: a Cut is {key2f(K1), key2f(K2 - 1)}, and the
// class of a ray height is the two compares of classify_cut.  K1 == K2 (never accepted) gives lo just above hi: still
// a monotone class, 0 or 2 everywhere.
//
// The heights a render can form are 0 and 2^-23 <= |cy| < 2^43 (fr_device.hpp, ScaleDiv); sqrt_rn and div_by_int are
// the correctly rounded operations only there.  The bisection runs over the keys of [-2^43, 2^43], and cut_height()
// maps the heights below 2^-23 in magnitude onto the zero of their sign (a non-decreasing map, so
// class(cut_height(cy)) is monotone over that whole range, and equal to class(cy) wherever a render looks).  Both ends
// of a Cut are then normal numbers or a zero.
//
// +-0: delta = fl(fl(cy a) + c1) - c2 with c1 = p1y^2 >= +0, so fl(cy a) + c1 is the same binary32 for cy = -0 and
// cy = +0; the linear t = (cy - p0y) / den is +-0 or the same non-zero number, and neither zero is < 0 or >= 1.  Hence
// class(-0) == class(+0) for every record: no cut falls between the two zeros, and the compares of classify_cut are
// plain float compares (under which -0 == +0) — they decide exactly as compares of the keys would.
struct Cut {
    float lo, hi;        // class 0 below lo, 2 above hi, 1 in [lo, hi]
};
__device__ __forceinline__ int classify_cut(const Cut &k, float cy)
{
    return cy > k.hi ? 2 : (cy < k.lo ? 0 : 1);
}
constexpr float CUT_HEIGHT_MIN = 1.1920929e-07f;         // 2^-23: the smallest non-zero |cy| of a render
constexpr float CUT_HEIGHT_MAX = 8796093022208.0f;       // 2^43
__device__ __forceinline__ float cut_height(float cy)
{
    return fabsf(cy) < CUT_HEIGHT_MIN ? __builtin_copysignf(0.0f, cy) : cy;
}
// the Cut of a candidate whose record is r: two bisections over the ordered keys, 2 x 32 evaluations of classify_row
__device__ inline Cut find_cut(const Rec &r)
{
    const uint32_t kmin = f2key(-CUT_HEIGHT_MAX), kmax = f2key(CUT_HEIGHT_MAX);
    auto first_at_least = [&](int T, uint32_t L) {        // smallest key in [L, kmax + 1] whose class is >= T
        uint32_t H = kmax + 1u;
        while (L < H) {
            const uint32_t mid = L + ((H - L) >> 1);
            if (classify_row(r, cut_height(key2f(mid))) >= T) H = mid; else L = mid + 1u;
        }
        return L;
    };
    const uint32_t K1 = first_at_least(1, kmin), K2 = first_at_least(2, K1);
    Cut k;
    k.lo = key2f(K1);
    k.hi = key2f(K2 - 1u);
    return k;
}

// the class a record build walks with: the reference's acceptance (FILL = 0) or the piece's (FILL = 1); CUT = 1: the
// reference's acceptance read off the candidate's row cut
template <int FILL, int CUT = 0>
__device__ __forceinline__ int row_class(const Rec &r, const Piece &pc, float cy, const Cut *k = nullptr)
{
    static_assert(!(FILL != 0 && CUT != 0), "row cuts hold the reference's acceptance only");
    if constexpr (FILL != 0) return classify_fill(pc, cy);
    else if constexpr (CUT != 0) return classify_cut(*k, cy);
    else return classify_row(r, cy);
}

// As build_record, but the bracket is this cell's exact sample-row range, written as integers
// into the lo / hi slots of the record (ra, re).  An empty range is ra = 1, re = 0.
// In three pieces, so that a set-up with lanes to spare can look at the four rows around the guessed
// ends in parallel (fr_c4.hpp): record_prep (fields + guesses), record_settle (the exact walk from the
// guesses), and their composition build_record_rows.
struct RowGuess {
    uint32_t ra, re;     // guessed first accepted row / first row past the range, clamped to [0, rows]
    bool empty;          // the candidate is discarded without a probe (see above)
};

// `drop`: the caller already knows that no row of the cell accepts the candidate (its row cut misses the cell's heights)
template <int FILL = 0>
__device__ __forceinline__ void record_prep(const int16_t *p, uint32_t root, const RowGeom &G, Rec &r, RowGuess &g, Piece *pc = nullptr, bool drop = false)
{
    const float p0x = (float)p[0], p0y = (float)p[1];
    const float p1x = (float)p[2], p1y = (float)p[3];
    const float p2x = (float)p[4], p2y = (float)p[5];
    const float a = p0y - 2 * p1y + p2y;                 // :48
    r.ax = p0x - 2 * p1x + p2x;                          // :53/:65
    r.bx = 2 * (p1x - p0x);
    r.p0x = p0x;
    r.sqsign = root ? 0x80000000u : 0u;
    const bool lin = a == 0.0f;                          // :49
    const float b = p0y - p1y;
    // ends of the accepted set in exact arithmetic: `start` is where t = 0 (or the vertex), `stop`
    // where t = 1 (or the vertex); the vertex and t = 0 are accepted, t = 1 is not
    bool empty;
    float c_start = p0y, c_stop = p2y;
    bool stop_incl = false;
    if (lin) {
        empty = (root != 0u) || (p2y == p0y);            // :50
        r.a = 0.0f; r.b = p0y; r.c1 = p2y - p0y; r.c2 = 0.0f;
        r.rden = 1.0f / r.c1;
        r.flags = REC_LINEAR | ((p0y < p2y) ? REC_LIN_MINUS : REC_LIN_PLUS);   // :55
    } else {
        r.a = a; r.b = b; r.c1 = p1y * p1y; r.c2 = p0y * p2y;        // :58, :60
        r.rden = 1.0f / a;
        r.flags = root ? REC_NEG_ROOT : 0u;
        const bool far_side = (root == 0u) == (a > 0.0f);            // this root satisfies (t - t_v) * 1 >= 0
        const bool tv_le0 = (b * a) <= 0.0f, tv_lt0 = (b * a) < 0.0f;     // a, b are integers: signs are exact
        const bool tv_ge1 = (a > 0.0f) ? (b >= a) : (b <= a);
        const float yv = p0y - (b * b) * r.rden;         // vertex height (a guess only: no second division)
        if (far_side) {
            empty = tv_ge1;
            if (!tv_le0) c_start = yv;
        } else {
            empty = tv_lt0;
            if (!tv_ge1) { c_stop = yv; stop_incl = true; }
        }
        if constexpr (FILL != 0) {
            // the piece: far side t in [max(0, t_v), 1], near side t in [0, min(1, t_v)] (t_v = b / a); its vertex end,
            // if any, is its lowest point when a > 0 and its highest when a < 0.  Near side with t_v = 0: a single point.
            const bool has_v = far_side ? !tv_le0 : !tv_ge1;
            if (!far_side && b == 0.0f) empty = true;
            const float other = far_side ? p2y : p0y;
            pc->a = a;
            pc->cv = (double)b * (double)b - (double)a * (double)p0y;
            pc->vend = has_v ? (a > 0.0f ? 1u : 2u) : 0u;
            pc->ylo = has_v ? (a > 0.0f ? yv : other) : fminf(p0y, p2y);
            pc->yhi = has_v ? (a > 0.0f ? other : yv) : fmaxf(p0y, p2y);
            if (!has_v && p0y == p2y) empty = true;
            c_start = pc->yhi; c_stop = pc->ylo;                    // (guesses: the first row below yhi, the first below ylo)
            stop_incl = true;
        }
    }
    if constexpr (FILL != 0) {
        if (lin) {
            pc->a = 1.0f; pc->cv = 0.0; pc->vend = 0u;
            pc->ylo = fminf(p0y, p2y); pc->yhi = fmaxf(p0y, p2y);
            c_start = pc->yhi; c_stop = pc->ylo;
            stop_incl = true;
        }
    }
    empty = empty || drop;
    g.empty = empty;
    g.ra = 1u; g.re = 0u;
    if (!empty) {
        // guesses: first row at / strictly below an end
        const float top = (float)G.rows;
        const bool start_hi = c_start >= c_stop;
        const float xh = G.row_of(start_hi ? c_start : c_stop), xl = G.row_of(start_hi ? c_stop : c_start);
        const bool hi_incl = (FILL != 0) ? false : (start_hi ? true : stop_incl), lo_incl = start_hi ? stop_incl : true;
        const float fa = hi_incl ? __builtin_ceilf(xh) : __builtin_floorf(xh) + 1.0f;    // first row accepted
        const float fe = lo_incl ? __builtin_floorf(xl) + 1.0f : __builtin_ceilf(xl);    // first row past it
        g.ra = (uint32_t)fminf(fmaxf(fa, 0.0f), top);
        g.re = (uint32_t)fminf(fmaxf(fe, 0.0f), top);
    }
}

// the exact ends from any starting guess: walk while the class of the row says so
template <int FILL = 0, int CUT = 0>
__device__ __forceinline__ void record_settle(const Rec &r, const RowGeom &G, uint32_t &ra, uint32_t &re, const Piece *pc = nullptr, const Cut *k = nullptr)
{
    auto classify_row = [&](const Rec &rr, float cy) {
        if constexpr (FILL != 0) return classify_fill(*pc, cy);
        else if constexpr (CUT != 0) return classify_cut(*k, cy);
        else return fr::classify_row(rr, cy);
    };
    // (one trip each when the guess is right: keep the compiler from unrolling them)
#pragma clang loop unroll(disable) vectorize(disable) interleave(disable)
    while (ra > 0u && classify_row(r, G.cy(ra - 1u)) <= 1) --ra;
#pragma clang loop unroll(disable) vectorize(disable) interleave(disable)
    while (ra < G.rows && classify_row(r, G.cy(ra)) == 2) ++ra;
    if (re < ra) re = ra;
#pragma clang loop unroll(disable) vectorize(disable) interleave(disable)
    while (re > ra && classify_row(r, G.cy(re - 1u)) == 0) --re;
#pragma clang loop unroll(disable) vectorize(disable) interleave(disable)
    while (re < G.rows && classify_row(r, G.cy(re)) >= 1) ++re;
}

// Bounds of the cell's ray heights: top >= cy(0), bot <= cy(rows - 1) — what a row cut is held against before any row is
// looked at.  Exact when the division is a multiply (scale = 2^k).  Otherwise the quotients are taken with v_rcp_f32
// (1 ulp) and one multiply instead of two IEEE divisions, and moved outwards by 2^-20 of their magnitude, eight times
// the error of the two roundings: a bound that is too wide only keeps a candidate that the walks then settle as empty.
struct RowSpan {
    float top, bot;
};
__device__ __forceinline__ RowSpan row_span(const RowGeom &G)
{
    const uint32_t last = G.rows ? G.rows - 1u : 0u;
    const float nt = (float)G.max_y - sub_off(0, G.n, G.phase);
    const float nb = (float)(G.max_y - (int32_t)(last / (uint32_t)G.n)) - sub_off((int)(last % (uint32_t)G.n), G.n, G.phase);
    RowSpan s;
    if (G.pow2) {
        s.top = nt * G.inv;
        s.bot = nb * G.inv;
    } else {
        const float rs = __builtin_amdgcn_rcpf(G.scale);
        const float t = nt * rs, b = nb * rs;
        s.top = __builtin_fmaf(fabsf(t), 9.5367431640625e-07f, t);
        s.bot = __builtin_fmaf(fabsf(b), -9.5367431640625e-07f, b);
    }
    return s;
}
// no row of the cell can have class 1: the cut is empty, lies wholly above the cell or wholly below it
__device__ __forceinline__ bool cut_misses(const Cut &k, const RowSpan &s)
{
    return !(k.lo <= k.hi) || k.hi < s.bot || k.lo > s.top;
}

template <int FILL = 0, int CUT = 0>
__device__ __forceinline__ void build_record_rows(const int16_t *p, uint32_t root, const RowGeom &G, Rec &r, const Cut *k = nullptr, const RowSpan *span = nullptr)
{
    RowGuess g;
    Piece pc;
    bool drop = false;
    if constexpr (CUT != 0) drop = cut_misses(*k, *span);
    record_prep<FILL>(p, root, G, r, g, &pc, drop);
    uint32_t ra = g.ra, re = g.re;
    if (!g.empty) record_settle<FILL, CUT>(r, G, ra, re, &pc, k);
    r.lo = __builtin_bit_cast(float, ra);
    r.hi = __builtin_bit_cast(float, re);
}


// FR_FILL_CONSISTENT form of build_record (prepare_kernel's records for the general kernel's large glyphs): the same
// fields, and [lo, hi] = the closed binary32 interval of the heights ylo <= cy < yhi that cross the piece, found by
// bisection over the ordered binary32 keys with the exact class (two times 32 steps per candidate).
__device__ inline bool build_record_fill(const int16_t *p, uint32_t root, Rec &r)
{
    RowGeom G;                                     // (no cell: record_prep's row guesses are not used)
    G.max_y = 0; G.scale = 1.0f; G.rows = 0u; G.n = 1; G.phase = 0;
    RowGuess g;
    Piece pc;
    record_prep<1>(p, root, G, r, g, &pc);
    if (g.empty) return false;
    const uint32_t kmin = f2key(-3.402823466e+38f), kmax = f2key(3.402823466e+38f);
    auto first_at_least = [&](int T) {            // smallest key whose class is >= T (the class is monotone)
        uint32_t L = kmin, H = kmax + 1u;
        while (L < H) {
            const uint32_t mid = L + ((H - L) >> 1);
            if (classify_fill(pc, key2f(mid)) >= T) H = mid; else L = mid + 1u;
        }
        return L;
    };
    const uint32_t LB = first_at_least(1), HB = first_at_least(2);
    if (LB >= HB) return false;
    r.lo = key2f(LB);
    r.hi = key2f(HB - 1u);
    return true;
}
}  // namespace fr

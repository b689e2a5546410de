// fr_prepare.hip — stand-alone per-glyph-set precompute of the root records (fr_records.hpp).
// Used at glyph-set creation (the records serve the render kernel's over-full rows and the SDF sign) and, per render,
// for glyphs too large for the render kernel's in-LDS record build.  Also the glyph set's row cuts (cut_kernel), found
// once at creation.
#include "fr_c4.hpp"

namespace fr {

// One wave64 per glyph.  Lane l builds candidate record c = base + l, where
// candidate 2s / 2s+1 are the t+ / t- roots of segment s (2s alone for a == 0);
// survivors (records whose bracket is not provably empty) are compacted with a ballot + prefix popcount into the glyph's slice
// [2*seg_start[g], ...) of the record arrays.
// FILL = 1: the records of FR_FILL_CONSISTENT (fr_records.hpp, build_record_fill)
template <int FILL>
__device__ __forceinline__ void prepare_body(const int16_t *__restrict__ pts,
                                                     const uint32_t *__restrict__ seg_p0,
                                                     const uint32_t *__restrict__ glyph_seg_start,
                                                     const uint32_t *__restrict__ glyph_list,
                                                     uint32_t n_glyphs,
                                                     Rec *__restrict__ out_recs,
                                                     uint32_t *__restrict__ glyph_rec_count)
{
    if (blockIdx.x >= n_glyphs) return;
    // the whole set (list == nullptr), or only the listed glyphs (a plan's glyphs of more than 128 segments)
    const uint32_t g = glyph_list ? glyph_list[blockIdx.x] : blockIdx.x;
    const uint32_t s0 = glyph_seg_start[g], s1 = glyph_seg_start[g + 1];
    const uint32_t n_cand = 2u * (s1 - s0);
    const uint32_t lane = threadIdx.x;
    const size_t out_base = 2u * (size_t)s0;
    uint32_t n_out = 0;
    for (uint32_t base = 0; base < n_cand; base += 64u) {
        const uint32_t c = base + lane;
        bool valid = false;
        Rec r;
        if (c < n_cand) valid = FILL ? build_record_fill(pts + 2u * (size_t)seg_p0[s0 + (c >> 1)], c & 1u, r) : build_record(pts + 2u * (size_t)seg_p0[s0 + (c >> 1)], c & 1u, r);
        const unsigned long long m = __ballot(valid);
        if (valid) {
            const uint32_t pos = n_out + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
            out_recs[out_base + pos] = r;
        }
        n_out += (uint32_t)__popcll(m);
    }
    if (lane == 0) glyph_rec_count[g] = n_out;
}
__global__ __launch_bounds__(64) void prepare_kernel(const int16_t *__restrict__ pts,
                                                     const uint32_t *__restrict__ seg_p0,
                                                     const uint32_t *__restrict__ glyph_seg_start,
                                                     const uint32_t *__restrict__ glyph_list,
                                                     uint32_t n_glyphs,
                                                     Rec *__restrict__ out_recs,
                                                     uint32_t *__restrict__ glyph_rec_count)
{
    prepare_body<0>(pts, seg_p0, glyph_seg_start, glyph_list, n_glyphs, out_recs, glyph_rec_count);
}
__global__ __launch_bounds__(64) void prepare_fill_kernel(const int16_t *__restrict__ pts,
                                                     const uint32_t *__restrict__ seg_p0,
                                                     const uint32_t *__restrict__ glyph_seg_start,
                                                     const uint32_t *__restrict__ glyph_list,
                                                     uint32_t n_glyphs,
                                                     Rec *__restrict__ out_recs,
                                                     uint32_t *__restrict__ glyph_rec_count)
{
    prepare_body<1>(pts, seg_p0, glyph_seg_start, glyph_list, n_glyphs, out_recs, glyph_rec_count);
}

// The row cuts of a glyph set (fr_records.hpp): thread c = 2 segment + root builds the candidate's record as the fast
// kernels' set-up does (record_prep, no cell) and bisects for its two cuts with classify_row.  A candidate that
// record_prep discards without a probe gets the empty cut {+inf, -inf}; the set-up discards it by the same rule and
// never reads the entry.  out: one float4 {lo0, hi0, lo1, hi1} per segment, written as two float2.
__global__ __launch_bounds__(256) void cut_kernel(const int16_t *__restrict__ seg_pts, uint32_t n_cand, float2 *__restrict__ out)
{
    const uint32_t c = blockIdx.x * 256u + threadIdx.x;
    if (c >= n_cand) return;
    RowGeom G;                                     // (no cell: record_prep's row guesses are not used)
    G.max_y = 0; G.scale = 1.0f; G.rows = 0u; G.n = 1; G.phase = 0;
    Rec r;
    RowGuess g;
    record_prep<0>(seg_pts + 6u * (size_t)(c >> 1), c & 1u, G, r, g);
    Cut k;
    k.lo = __builtin_inff(); k.hi = -__builtin_inff();
    if (!g.empty) k = find_cut(r);
    out[c] = make_float2(k.lo, k.hi);
}

// The candidate table of a glyph set (Cand, fr_c4.hpp), after cut_kernel: one wave per glyph.  Lane l takes candidates
// l, l + 64, ... of the glyph, builds each one's record as the set-up does (record_prep, no cell) and reads its cut; a
// candidate is live when record_prep keeps it and its cut is not empty.  A first walk counts the live quadratic
// candidates; the second writes every live candidate to its place in record order — quadratic first, linear last, each
// group in candidate order: a ballot and a prefix count per 64 candidates — and the dead slots behind them.
__global__ __launch_bounds__(64) void cand_kernel(const int16_t *__restrict__ seg_pts, const uint32_t *__restrict__ glyph_seg_start,
                                                  const float2 *__restrict__ cuts, uint32_t n_glyphs, Cand *__restrict__ out)
{
    const uint32_t gl = blockIdx.x, lane = threadIdx.x;
    if (gl >= n_glyphs) return;
    const uint32_t s0 = glyph_seg_start[gl], n_cand = 2u * (glyph_seg_start[gl + 1u] - s0);
    const size_t base = 2u * (size_t)s0;
    RowGeom G;                                     // (no cell: record_prep's row guesses are not used)
    G.max_y = 0; G.scale = 1.0f; G.rows = 0u; G.n = 1; G.phase = 0;
    const unsigned long long below = (1ull << lane) - 1ull;
    uint32_t n_quad = 0u;
    for (uint32_t c0 = 0u; c0 < n_cand; c0 += 64u) {
        const uint32_t c = c0 + lane;
        bool quad = false;
        if (c < n_cand) {
            Rec r;
            RowGuess g;
            record_prep<0>(seg_pts + 6u * (size_t)(s0 + (c >> 1)), c & 1u, G, r, g);
            const float2 q = cuts[base + c];
            quad = !g.empty && q.x <= q.y && (int32_t)r.flags >= 0;
        }
        n_quad += (uint32_t)__popcll(__ballot(quad));
    }
    uint32_t at_q = 0u, at_l = n_quad;
    for (uint32_t c0 = 0u; c0 < n_cand; c0 += 64u) {
        const uint32_t c = c0 + lane;
        bool live = false, lin = false;
        Cand e;
        if (c < n_cand) {
            Rec r;
            RowGuess g;
            record_prep<0>(seg_pts + 6u * (size_t)(s0 + (c >> 1)), c & 1u, G, r, g);
            const float2 q = cuts[base + c];
            live = !g.empty && q.x <= q.y;
            lin = (int32_t)r.flags < 0;
            e.rec = c4_make_rec40<0>(r, 0u, 0u);
            e.cut.lo = q.x; e.cut.hi = q.y;
        }
        const unsigned long long mq = __ballot(live && !lin), ml = __ballot(live && lin);
        if (live) out[base + (lin ? at_l + (uint32_t)__popcll(ml & below) : at_q + (uint32_t)__popcll(mq & below))] = e;
        at_q += (uint32_t)__popcll(mq);
        at_l += (uint32_t)__popcll(ml);
    }
    Cand dead;
    dead.rec.a = dead.rec.b = dead.rec.c1 = dead.rec.c2 = dead.rec.ax = dead.rec.bx = dead.rec.p0x = dead.rec.rden = dead.rec.sgn = 0.0f;
    dead.rec.fr = 0u;
    dead.cut.lo = __builtin_inff(); dead.cut.hi = -__builtin_inff();
    for (uint32_t c = at_l + lane; c < n_cand; c += 64u) out[base + c] = dead;
}

void launch_cands(const int16_t *seg_pts, const uint32_t *glyph_seg_start, const float4 *cuts, uint32_t n_glyphs, uint4 *out, hipStream_t stream)
{
    if (n_glyphs == 0) return;
    hipLaunchKernelGGL(cand_kernel, dim3(n_glyphs), dim3(64), 0, stream, seg_pts, glyph_seg_start, reinterpret_cast<const float2 *>(cuts),
                       n_glyphs, reinterpret_cast<Cand *>(out));
}

void launch_cuts(const int16_t *seg_pts, uint32_t n_seg, float4 *out, hipStream_t stream)
{
    if (n_seg == 0) return;
    const uint32_t n_cand = 2u * n_seg;
    hipLaunchKernelGGL(cut_kernel, dim3((uint32_t)(((uint64_t)n_cand + 255u) / 256u)), dim3(256), 0, stream, seg_pts, n_cand, reinterpret_cast<float2 *>(out));
}

void launch_prepare(const int16_t *pts, const uint32_t *seg_p0, const uint32_t *glyph_seg_start,
                    const uint32_t *glyph_list, uint32_t n_glyphs, Rec *out_recs, uint32_t *glyph_rec_count,
                    hipStream_t stream, int fill)
{
    if (n_glyphs == 0) return;
    hipLaunchKernelGGL(fill ? prepare_fill_kernel : prepare_kernel, dim3(n_glyphs), dim3(64), 0, stream, pts, seg_p0,
                       glyph_seg_start, glyph_list, n_glyphs, out_recs, glyph_rec_count);
}

}  // namespace fr

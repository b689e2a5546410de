// fr_text_mask_kernel.inc — one instance's n^2-bit non-zero mask at pixel (X, Y), included inside the instance loops of
// fr_text_cover_kernel.inc and fr_text_colour_kernel.inc.  Uses N, FILL, PLACE, a, rn, in, X, Y, off[N]; sets m (bit j*N + i: the
// winding at sub-sample (i, j) is non-zero).  Text, not a function: as a function taking the instance by reference it
// moved five n = 4 instances to another VGPR bracket (DESIGN.md 4.7).
// The map from a sample to the glyph's font units (include/fr_raster.h):
//     !PLACE (TextInst):    cy = (f32(pen_y - Y) - off(j)) / s,            cx = t,           s the run's scale
//      PLACE (TextInstEx):  cy = (f32(iy - Y) + (fy - off(j))) / s,        cx = t - k * cy,  s and k the placement's
//     t = (f32(X - ix) + (off(i) - fx)) / s: off(i) - fx is exact (multiples of 1/64 in (-1, 1))
// s, k, cy[j] and k * cy[j] are the same in all lanes (scalar registers); per lane there are t[i], and under PLACE the n^2
// abscissae are subtracted at every accepted root rather than held as a table of n^2 floats (which costs a wave per SIMD
// at n = 4 and measured slower: DESIGN.md 4.7).
            float s;
            if constexpr (PLACE) s = in.scale;
            else s = rn.scale;
            const float xf = (float)(X - in.ix);
            const float fx = (float)in.fx64 * 0.015625f;
            [[maybe_unused]] float fy = 0.0f;
            if constexpr (PLACE) fy = (float)in.fy64 * 0.015625f;
            float t[N];
#pragma unroll
            for (int i = 0; i < N; ++i) t[i] = (xf + (off[i] - fx)) / s;
            float cy[N];
            [[maybe_unused]] float kcy[N];
#pragma unroll
            for (int j = 0; j < N; ++j) {
                if constexpr (PLACE) {
                    cy[j] = ((float)(in.iy - Y) + (fy - off[j])) / s;
                    kcy[j] = in.slant * cy[j];
                } else {
                    cy[j] = ((float)(in.pen_y - Y) - off[j]) / s;
                }
            }
            int wn[N * N];
#pragma unroll
            for (int k = 0; k < N * N; ++k) wn[k] = 0;
            const Rec *recs = a.recs + in.rec;
            const uint32_t nr = a.rec_count[in.glyph];
            for (uint32_t r = 0; r < nr; ++r) {
                const Rec rc = recs[r];
#pragma unroll
                for (int j = 0; j < N; ++j) {
                    if (cy[j] >= rc.lo && cy[j] <= rc.hi) {                // [lo, hi] contains the accepted heights
                        float xx;
                        int sgn;
                        if (rec_cross<FILL>(rc, cy[j], xx, sgn)) {
                            if constexpr (PLACE) {
                                float kc = kcy[j];
                                asm volatile("" : "+v"(kc));               // (keeps the subtracts here: without it they are
                                                                           // hoisted out of the record loop into that table)
#pragma unroll
                                for (int i = 0; i < N; ++i) wn[j * N + i] += !(xx < t[i] - kc) ? sgn : 0;
                            } else {
#pragma unroll
                                for (int i = 0; i < N; ++i) wn[j * N + i] += !(xx < t[i]) ? sgn : 0;
                            }
                        }
                    }
                }
            }
            m = 0u;
#pragma unroll
            for (int k = 0; k < N * N; ++k) m |= (wn[k] != 0 ? 1u : 0u) << k;

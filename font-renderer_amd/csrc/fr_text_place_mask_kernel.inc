// fr_text_place_mask_kernel.inc — fr_text_mask_kernel.inc for a TextInstEx: one instance's n^2-bit non-zero mask at pixel
// (X, Y) under the placement's own sample map (include/fr_raster.h, fr_glyph_place_ex), included inside the instance
// loops of fr_text_place.hip.  Uses N, FILL, a, in, X, Y, off[N]; defines m (bit j*N + i: the winding at sub-sample
// (i, j) is non-zero).  The scale s, the slant k, cy[j] and k * cy[j] are the same in all lanes (scalar registers); per
// lane there are t[i] and the n^2 abscissae cx = t[i] - k * cy[j], subtracted at every accepted root rather than held as a
// table of n^2 floats (which costs a wave per SIMD at n = 4 and measured slower: DESIGN.md 4.7).  The records and
// rec_cross are the text kernels' own.
            const float s = in.scale, kk = in.slant;
            const float xf = (float)(X - in.ix);
            const float fx = (float)in.fx64 * 0.015625f, fy = (float)in.fy64 * 0.015625f;
            float t[N];
#pragma unroll
            for (int i = 0; i < N; ++i) t[i] = (xf + (off[i] - fx)) / s;
            float cy[N], kcy[N];
#pragma unroll
            for (int j = 0; j < N; ++j) {
                cy[j] = ((float)(in.iy - Y) + (fy - off[j])) / s;
                kcy[j] = kk * cy[j];
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
                            float kc = kcy[j];
                            asm volatile("" : "+v"(kc));                   // (keeps the subtracts here: without it they are
                                                                           // hoisted out of the record loop into that table)
#pragma unroll
                            for (int i = 0; i < N; ++i) wn[j * N + i] += !(xx < t[i] - kc) ? sgn : 0;
                        }
                    }
                }
            }
            uint32_t m = 0u;
#pragma unroll
            for (int k = 0; k < N * N; ++k) m |= (wn[k] != 0 ? 1u : 0u) << k;

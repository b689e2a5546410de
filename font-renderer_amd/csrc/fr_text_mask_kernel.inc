// fr_text_mask_kernel.inc — one instance's n^2-bit non-zero mask at pixel (X, Y), included inside the instance loops of
// text_kernel and text_rgba_kernel (fr_text.hip).  Uses N, FILL, a, in, X, Y, off[N], scale; defines m (bit j*N + i:
// the winding at sub-sample (i, j) is non-zero).  Included as it is, text_kernel's code generation is unchanged.
            // cx = (f32(X - ix) + (off(i) - fx)) / scale: off(i) - fx is exact (multiples of 1/64 in (-1, 1))
            const float xf = (float)(X - in.ix);
            const float fx = (float)in.fx64 * 0.015625f;
            float cx[N];
#pragma unroll
            for (int i = 0; i < N; ++i) cx[i] = (xf + (off[i] - fx)) / scale;
            float cy[N];
#pragma unroll
            for (int j = 0; j < N; ++j) cy[j] = ((float)(in.pen_y - Y) - off[j]) / scale;
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
#pragma unroll
                            for (int i = 0; i < N; ++i) wn[j * N + i] += !(xx < cx[i]) ? sgn : 0;
                        }
                    }
                }
            }
            uint32_t m = 0u;
#pragma unroll
            for (int k = 0; k < N * N; ++k) m |= (wn[k] != 0 ? 1u : 0u) << k;

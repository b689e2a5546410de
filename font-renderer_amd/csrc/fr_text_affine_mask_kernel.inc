// fr_text_affine_mask_kernel.inc — one fr_glyph_place_affine instance's n^2-bit non-zero mask at pixel (X, Y): the sibling
// of fr_text_mask_kernel.inc, included by the two row bodies for TextInstAffine.  Uses N, FILL, a, in, X, Y, inside, off[N];
// sets m (bit j*N + i: the winding at sub-sample (i, j) is non-zero).
// The map from a sample to the glyph's font units (include/fr_raster.h), one rounding per operation:
//     dx = f32(X - ix) + (off(i) - fx),   dy = f32(iy - Y) + (fy - off(j))        (both brackets exact)
//     cx = f32(q00 * dx) + f32(q01 * dy), cy = f32(q10 * dx) + f32(q11 * dy)
// cy differs per lane, so every lane solves every record at its own height: rec_cross with the lane's cy, n^2 roots per
// record and lane where the upright forms pay n per wave.  The four products are held (2n per lane, 2n wave-uniform) and
// the sums are formed where they are used, which is the definition's rounding and keeps 2 n^2 floats from being live.
// The cull: [cmin, cmax] is the range of the cy values the lanes inside the cell use (f2key makes the floats ordered
// integers, the DPP scan of fr_wave.hpp reduces them); a record whose [lo, hi] misses it is accepted by no sample, so
// skipping it (a wave-uniform branch on scalar registers) cannot change a byte.  Lanes outside the cell are left out of
// the range: their mask is not used.  At small angles a wave row spans few font units in y and most records fall away.
            const float xf = (float)(X - in.ix), yf = (float)(in.iy - Y);
            const float fx = (float)in.fx64 * 0.015625f, fy = (float)in.fy64 * 0.015625f;
            float ax[N], bx[N], ay[N], by[N];
#pragma unroll
            for (int i = 0; i < N; ++i) {
                const float dx = xf + (off[i] - fx);
                ax[i] = in.q00 * dx;
                bx[i] = in.q10 * dx;
            }
#pragma unroll
            for (int j = 0; j < N; ++j) {
                const float dy = yf + (fy - off[j]);
                ay[j] = in.q01 * dy;
                by[j] = in.q11 * dy;
            }
            uint32_t kmax = 0u, kmin = 0u;                                 // (kmin: the maximum of ~key)
            if (inside) {
#pragma unroll
                for (int j = 0; j < N; ++j) {
#pragma unroll
                    for (int i = 0; i < N; ++i) {
                        const uint32_t k = f2key(bx[i] + by[j]);
                        kmax = max(kmax, k);
                        kmin = max(kmin, ~k);
                    }
                }
            }
            // (no lane inside: both keys stay 0, both bounds are NaN and every record is skipped)
            const float cmax = key2f((uint32_t)__builtin_amdgcn_readlane((int)wave_incl_max(kmax), 63));
            const float cmin = key2f(~(uint32_t)__builtin_amdgcn_readlane((int)wave_incl_max(kmin), 63));
            int wn[N * N];
#pragma unroll
            for (int k = 0; k < N * N; ++k) wn[k] = 0;
            const Rec *recs = a.recs + in.rec;
            const uint32_t nr = a.rec_count[in.glyph];
            for (uint32_t r = 0; r < nr; ++r) {
                const Rec rc = recs[r];
                if (!(rc.hi >= cmin && rc.lo <= cmax)) continue;           // (wave-uniform) no sample of this row is in [lo, hi]
#pragma unroll
                for (int j = 0; j < N; ++j) {
#pragma unroll
                    for (int i = 0; i < N; ++i) {
                        const float cy = bx[i] + by[j];
                        if (cy >= rc.lo && cy <= rc.hi) {                  // [lo, hi] contains the accepted heights
                            float xx;
                            int sgn;
                            if (rec_cross<FILL>(rc, cy, xx, sgn)) wn[j * N + i] += !(xx < ax[i] + ay[j]) ? sgn : 0;
                        }
                    }
                }
            }
            m = 0u;
#pragma unroll
            for (int k = 0; k < N * N; ++k) m |= (wn[k] != 0 ? 1u : 0u) << k;

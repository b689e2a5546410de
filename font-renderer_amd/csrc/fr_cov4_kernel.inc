// fr_cov4_kernel.inc — the body of cov4_kernel (fr_cov4.hip), included by its two kernel templates (FILL = 0 / 1).
    using L = C4Lds<WLOG, RPL, NS, CAP>;
    constexpr uint32_t LSTRIDE = L::LSTRIDE;
    static_assert(NS == 4 || NS == 2, "samples per axis");
    constexpr uint32_t RCAP = L::RCAP;
    constexpr uint32_t NW = C4_WAVES;
    constexpr uint32_t SW = 16u << WLOG;            // strip width, pixels
    constexpr uint32_t NCOL = SW * (uint32_t)NS;    // sample columns
    constexpr uint32_t NWIN = 1u << WLOG;           // 16-pixel windows per pixel row
    constexpr uint32_t PRB = L::PRB;                // pixel rows per wave band
    constexpr int LN = (NS == 4) ? 2 : 1;           // log2 NS
    // SPLIT: the instances of many records (glyphs of > 256 segments: wiggly outlines whose over-full rows come dozens to
    // a band) can walk a band's pairs again in two halves of the sample columns — a 64-crossing tier out of two 32-slot
    // passes, no LDS of its own (below) — instead of settling every over-full row by its own direct sum
    constexpr bool SPLIT = RPL >= 8 && CAP == 32;
    extern __shared__ __align__(16) unsigned char smem[];

    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    // (the wave index as a SCALAR: everything a band derives from it — rows, ray heights' base, the output address — is then
    // scalar arithmetic and the stores take the band's base from SGPRs; `tid >> 6` alone is a vector value to the compiler)
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid >> 6));
    uint32_t bid = blockIdx.x, strip = 0, bgrp = 0;
    if (A.strips != 1u) { strip = bid % A.strips; bid /= A.strips; }
    if (A.band_groups != 1u) { bgrp = bid % A.band_groups; bid /= A.band_groups; }
    const uint32_t jidx = bid;
    C4_ABL_LAUNCH_ONLY();
    const Job job = A.jobs[jidx];
    const uint32_t x0s = strip * SW;
    const uint32_t band_first = bgrp * A.bands_per_wg;
    if (band_first * PRB >= job.h || x0s >= job.w) return;                  // workgroup-uniform
    const uint32_t band_end = min(band_first + A.bands_per_wg, (job.h + PRB - 1u) / PRB);
    const uint32_t wlim = min(SW, job.w - x0s);                             // pixels of this strip that lie in the cell
    const int phase = A.phase_center;
    const uint32_t seg0 = A.job_seg[2u * (size_t)jidx], nseg = A.job_seg[2u * (size_t)jidx + 1u];
    C4_ABL_JOB_ONLY();
    C4_ABL_SEGLOAD_ONLY();
    float *s_cxp = reinterpret_cast<float *>(smem);
    Rec40 *s_rec = reinterpret_cast<Rec40 *>(smem + L::CX);
    unsigned char *wregion = smem + L::OFF_WAVES + (size_t)wave * L::WAVE;
    uint32_t *s_wcnt = reinterpret_cast<uint32_t *>(smem + L::OFF_WCNT);

    uint32_t *const s_next_band = s_wcnt + 15;                              // (the set-up's barriers order this store)
    if (tid == 0u) *s_next_band = band_first + NW;
    const uint32_t rec_cnt = c4_setup<NW, RCAP, NS, NCOL, FILL>(A, job, seg0, nseg, x0s, phase, s_cxp, s_rec, s_wcnt, reinterpret_cast<uint32_t *>(smem + L::OFF_WAVES));
    const int32_t min_xs = job.min_x + (int32_t)x0s;
    const ScaleDiv sdiv = scale_div(job.scale);     // (workgroup-uniform: the bands' ray heights multiply when scale is a power of two)
    const float jscale = job.scale * (float)NS;
    const float joff = (float)min_xs * (float)NS + (phase ? 0.5f : 0.0f) - 1.0f;
    const float ncolf = (float)NCOL;
    // every lane keeps the row ranges of its records in registers for all its bands: records RPL*lane ...
    // (consecutive, so the record index grows along the pair sequence and the marker decode is a max-scan)
    const bool few = RPL == 2 || rec_cnt <= 128u;   // (RPL == 2: the plan sends only glyphs of <= 128 candidate roots)              // workgroup-uniform: two records per lane are enough
    const uint32_t per = few ? 2u : (uint32_t)RPL;
    uint32_t rra[RPL], rre[RPL];
#pragma unroll
    for (int i = 0; i < RPL; ++i) {
        const uint32_t k = per * lane + (uint32_t)i;
        const bool have = k < rec_cnt && (!few || i < 2);
        const uint32_t f = s_rec[have ? k : 0u].fr;
        rra[i] = have ? (f & 0xfffu) : 1u;
        rre[i] = have ? ((f >> 12) & 0xfffu) : 0u;
    }

    uint16_t *s_lists = reinterpret_cast<uint16_t *>(wregion);
    uint16_t *s_pairs = reinterpret_cast<uint16_t *>(wregion + L::OFF_PAIRS);
    float *s_cy = reinterpret_cast<float *>(wregion + L::OFF_CY);
    uint32_t *s_cnt = reinterpret_cast<uint32_t *>(wregion + L::OFF_CNT);
    int16_t *s_roff = reinterpret_cast<int16_t *>(wregion + L::OFF_ROFF);
    unsigned char *s_E = wregion;
    // The pair walk forms its LDS addresses from pre-scaled indices (below): base + index, one add each.  Where the register
    // budget allows the wave region's offset is kept in a VGPR — an opaque copy — so that the add is a VOP2 of two VGPRs,
    // the fast class of DESIGN.md section 4.0; with the base in an SGPR the same add is a normal-class instruction.  Not in
    // the six-workgroup instances (held to 80 VGPRs) nor in the 512-record ones, which fill their 168 registers as it is:
    // the copy took their scratch from 8 to 16 bytes per lane.
    constexpr bool VBASE = c4_occ(CAP, WLOG, RPL) <= 4 && RPL != 8;
    uint32_t wreg = L::OFF_WAVES + wave * L::WAVE;
    if constexpr (VBASE) asm volatile("" : "+v"(wreg));
    const uint32_t lane4 = lane << 2;
    const uint32_t mk0 = 2u * (per * lane + 1u);       // the marker of my first record: 2 (k + 1)
    static_assert(LSTRIDE % 2u == 0u && C4_PCAP % 64 == 0, "row lists are whole dwords; chunks are whole trips");

    C4_ABL_SETUP_ONLY();
    // (no workgroup barrier below: waves are independent.)  Every wave starts on band `wave` of the group and then takes
    // the next band nobody has started yet (one LDS counter): bands differ a lot in cost — the margins above and below the
    // glyph are nearly free — and a workgroup keeps its LDS until its slowest wave is done.  (Measured, same box: C3 - 1.7 %,
    // S = 256 - 6 %, configs[3]'s shard - 1 %; win1_kernel keeps the static round-robin: on its large cells the dealing was
    // worth 0.3 %.)
#if FR_DYN_BANDS
    for (uint32_t band = band_first + wave; band < band_end;
         band = (uint32_t)__builtin_amdgcn_readfirstlane((int)(lane == 0u ? atomicAdd(s_next_band, 1u) : 0u))) {
#else
    for (uint32_t band0 = band_first; band0 < band_end; band0 += NW) {
        const uint32_t band = band0 + wave;
        if (band >= band_end) break;
#endif
        const uint32_t y0 = band * PRB;
        const uint32_t row_b0 = band * 64u;
        // ray height of sample row `lane` of the band: cy = (f32(max_y - y) - off(jj)) / scale  (:27)
        const float cy = sdiv((float)(job.max_y - (int32_t)(y0 + (lane >> LN))) - sub_off((int)(lane & (uint32_t)(NS - 1)), NS, phase));
        uint16_t *mylist = s_lists + lane * LSTRIDE;
        auto init_lists = [&]() {
            const uint4 ones = make_uint4(0xfffdfffdu, 0xfffdfffdu, 0xfffdfffdu, 0xfffdfffdu);
#pragma unroll
            for (uint32_t q = 0; q < CAP / 8u; ++q) c4_st16<LSTRIDE>(mylist + 8u * q, ones);
            s_cnt[lane] = 0u;
        };
        init_lists();
        s_cy[lane] = cy;

        // ---- layout + evaluation.  The band's (record, row) pairs form ONE sequence, record by record (lane by lane,
        // a lane's records in order); it is walked in chunks of PCAP pairs — only the markers are per chunk, the row
        // offsets and the running record index carry over — 64 pairs per trip, every trip but the last one full.
        uint32_t c[RPL], off0 = 0u, tot;
        {
            uint32_t r0[RPL], csum = 0;
            {
                const uint32_t lo = row_b0, hi = row_b0 + 64u;
#pragma unroll
                for (int i = 0; i < RPL; ++i) {
                    r0[i] = max(rra[i], lo);
                    const uint32_t r1 = min(rre[i], hi);
                    c[i] = r1 > r0[i] ? r1 - r0[i] : 0u;
                    csum += c[i];
                }
            }
            const uint32_t incl = wave_incl_add(csum);
            tot = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
            if (tot) {
                off0 = incl - csum;
                {
                    uint32_t off = off0, ro[RPL];
#pragma unroll
                    for (int i = 0; i < RPL; ++i) {
                        // (a pair's row is only ever used mod 64: kept as the byte offset of the row's dword, 4 (row & 63))
                        ro[i] = ((r0[i] - row_b0 - off) & 63u) << 2;
                        off += c[i];
                    }
                    // my records' row offsets sit side by side: one store
                    if (few) *reinterpret_cast<uint32_t *>(s_roff + 2u * lane) = ro[0] | (ro[1] << 16);
                    else if constexpr (RPL == 4) *reinterpret_cast<uint2 *>(s_roff + 4u * lane) = make_uint2(ro[0] | (ro[1] << 16), ro[2] | (ro[3] << 16));
                    else if constexpr (RPL >= 8) {
#pragma unroll
                    for (int q8 = 0; q8 < RPL / 8; ++q8)
                        reinterpret_cast<uint4 *>(s_roff + (uint32_t)RPL * lane)[q8] = make_uint4(ro[8 * q8] | (ro[8 * q8 + 1] << 16), ro[8 * q8 + 2] | (ro[8 * q8 + 3] << 16),
                                                                                                  ro[8 * q8 + 4] | (ro[8 * q8 + 5] << 16), ro[8 * q8 + 6] | (ro[8 * q8 + 7] << 16));
                }
                }
            }
        }
        // one walk of the band's pairs; SPLIT instances can walk again keeping only the crossings with J - 1 in
        // [jlo, jlo + jspan) (every instance's first walk keeps J in 1 .. NCOL: all but the ones left of the strip)
        auto eval_pass = [&](uint32_t jlo, uint32_t jspan) {
            (void)jlo; (void)jspan;
            if (tot) {
                const uint32_t npairs = tot;
                uint32_t carry = 0u;               // record index (+ 1) of the last pair walked so far
              for (uint32_t base = 0; base < npairs; base += (uint32_t)C4_PCAP) {
                // markers: slot `off - base` of the chunk holds 2 (k + 1) where record k's run starts, 0 elsewhere
                // (monotone in k like k + 1, and at once the byte offset of the record's row offset — and half its record's)
                if (C4_PCAP >= 512 || lane < C4_PCAP / 8) reinterpret_cast<uint4 *>(s_pairs)[lane] = make_uint4(0, 0, 0, 0);
                wave_lds_sync();
                {
                    uint32_t off = off0 - base;    // (wraps below the chunk: an unsigned compare takes both ends)
#pragma unroll
                    for (int i = 0; i < RPL; ++i) {
                        if (c[i] && off < (uint32_t)C4_PCAP) s_pairs[off] = (uint16_t)(mk0 + 2u * (uint32_t)i);
                        off += c[i];
                    }
                }
                wave_lds_sync();
                const uint32_t nhere = min(npairs - base, (uint32_t)C4_PCAP);
                // one pair per lane per trip; the marker max-scan of the NEXT 64 pairs is issued before the
                // current 64 are evaluated (an independent chain that fills the evaluation's wait states)
                uint32_t k_cur = max(wave_incl_max((uint32_t)s_pairs[lane]), carry);
                carry = (uint32_t)__builtin_amdgcn_readlane((int)k_cur, 63);
                // (the byte offset of my marker of the next trip is a vector register advanced by a literal, not rebuilt
                // from the scalar trip counter every trip)
                uint32_t pn2 = 2u * lane + 128u;
                for (uint32_t p0 = 0; p0 < nhere && C4_ABL_KEEP(3); p0 += 64u) {
                    const uint32_t s_next = wave_incl_max((uint32_t)*reinterpret_cast<const uint16_t *>(smem + (wreg + min(pn2, 2u * (uint32_t)C4_PCAP - 2u)) + L::OFF_PAIRS));
                    pn2 += 128u;
                    {
                        const uint32_t k2 = k_cur;                              // 2 (record index + 1)
                        // pair base + p0 + lane of npairs (p0 < nhere: the scalar side does not wrap)
                        const bool livep = lane < npairs - base - p0;
                        // (a lane past the end decodes the last record and a row that may lie outside the band:
                        // it computes like the others and is kept from the table walk and the append)
#if C4_ABL_NODECODE
                        const uint32_t row4 = (lane4 + ((k2 & 2u) << 1)) & 252u;                    // timing-only: no dependent decode loads
                        const uint32_t raddr = L::CX + ((lane & 3u) + (A.n_jobs == 0xffffffffu ? (k2 >> 1) : 0u)) * (uint32_t)sizeof(Rec40);
#else
                        // row = pair index + the record's row offset, mod 64 — and the pair index is my lane mod 64 (chunks and
                        // trips are multiples of 64): 4 row is the byte offset of s_cy[row] and s_cnt[row]
                        const uint32_t roff4 = *reinterpret_cast<const uint16_t *>(smem + (wreg + k2) + (L::OFF_ROFF - 2u));
                        const uint32_t row4 = (lane4 + roff4) & 252u;
                        // (one 24-bit multiply-add for the record's LDS address, small offsets for its five 8-byte reads)
                        const uint32_t raddr = __umul24(k2, (uint32_t)sizeof(Rec40) / 2u) + (L::CX - (uint32_t)sizeof(Rec40));
#endif
                        // (k2 is even, so the address is a multiple of 8 like every record's: said to the compiler, which
                        // otherwise reads the record in 4-byte pieces)
                        const Rec40 r = *reinterpret_cast<const Rec40 *>(__builtin_assume_aligned(smem + raddr, 8));
                        const uint32_t rowa = wreg + row4;
                        const float cyr = *reinterpret_cast<const float *>(smem + rowa + L::OFF_CY);
                        // KIND 1 = all quadratic, 2 = all linear (no delta, no square root), 0 = mixed (both + a select).
                        // Only KIND 0 is built: single-kind trips saved 87 vector instructions per wave on C3 but ran 2 % slower
                        // (58 more branches); the body keeps its KIND-generic shape, which fixes its code generation.
                        const unsigned long long linm = __builtin_amdgcn_sicmp((int32_t)r.fr, 0, 40 /* ICMP_SLT */);
                        auto body = [&](auto kind) {
                            constexpr int KIND = decltype(kind)::value;
                            // the reference's operation order, one rounding per operation (:51, :58-61, :53/:65, :67);
                            // the row range [ra, re) is exactly the set of rows on which the reference accepts this
                            // root (fr_records.hpp), so its three rejection tests (:52, :59, :64) are not repeated
                            float num;
                            if (KIND == 2) {
                                num = cyr - r.b;
                            } else {
                                const float delta0 = cyr * r.a + r.c1 - r.c2;
                                // (FILL: a crossing row can lie a few ulps past the rounded delta = 0 — clamp, no NaN)
                                const float delta = FILL ? __builtin_fmaxf(delta0, 0.0f) : delta0;
                                const float sq = sqrt_rn(delta);
                                const float numq = r.b + sq * r.sgn;
                                num = (KIND == 1) ? numq : c4_self(linm, cyr - r.b, numq);
                            }
                            const float t = div_by_int(num, r.a, r.rden);
                            const float xx = (r.ax * t + r.bx) * t + r.p0x;
                            uint32_t code;
                            if (KIND == 2) {
                                code = (r.fr >> 24) & 3u;                              // (:55)
                            } else {
                                const float dy = r.a * t - r.b;                        // (:67)
                                if (KIND == 1) code = FILL ? ((r.fr >> 24) & 3u) : ((dy > 0.0f) ? 0u : 2u);   // (:68)
                                else code = (dy > 0.0f) ? ((r.fr >> 26) & 3u) : ((r.fr >> 24) & 3u);
                            }
                            // J = #{ j in [0, ncol) : cx(j) <= xx }   (:54, :66) — guess, one paired read, rare walk
                            const float gf = __builtin_amdgcn_fmed3f(__builtin_fmaf(xx, jscale, -joff), 0.0f, ncolf);
                            int J = (int)gf;
                            {
                                const float c0 = s_cxp[J], c1 = s_cxp[J + 1];
                                const bool good = (c0 <= xx) & (xx < c1);
                                if (__builtin_expect(!good & livep, 0)) {
                                    while (s_cxp[J + 1] <= xx) ++J;
                                    while (s_cxp[J] > xx) --J;
                                }
                            }
                            bool keep = livep & (J > 0);
                            if constexpr (SPLIT) keep = livep & ((uint32_t)(J - 1) - jlo < jspan);
                            if (keep) {
                                const uint32_t pos = atomicAdd(reinterpret_cast<uint32_t *>(smem + rowa + L::OFF_CNT), 1u);
                                uint16_t *rowlist = reinterpret_cast<uint16_t *>(smem + (wreg + __umul24(row4, LSTRIDE / 2u)));
                                rowlist[min(pos, (uint32_t)CAP)] = (uint16_t)(((uint32_t)J << 2) | code);   // (slot CAP: the dump)
                            }
                        };
                        body(std::integral_constant<int, 0>{});
                    }
                    k_cur = max(s_next, carry);
                    carry = (uint32_t)__builtin_amdgcn_readlane((int)k_cur, 63);
                }
                wave_lds_sync();
              }
            }
        };
        eval_pass(0u, NCOL);
        C4_ABL_EVAL_ONLY();
        uint32_t cnt = s_cnt[lane];
        uint8_t *const out_band = reinterpret_cast<uint8_t *>(A.out) + ((size_t)job.out_y + y0) * A.out_stride + job.out_x + x0s;
        const uint32_t wx = lane & (NWIN - 1u);
        // pixel rows of this band that lie in the cell; `edge`: the band or the strip is cut by the cell's border
        // (wave-uniform — a whole cell never takes the clipped stores)
        const uint32_t hlim = min(PRB, job.h - y0);
                const bool edge = __builtin_amdgcn_readfirstlane((int)((wlim < SW) | (hlim < PRB))) != 0;
        if (__ballot(cnt != 0u) == 0ull) {
            // no crossing on any of my 64 sample rows: every winding is 0 — store the band's background
            for (uint32_t yl = lane >> WLOG; yl < PRB; yl += (64u >> WLOG)) {
                const uint4 z = make_uint4(0, 0, 0, 0);
                unsigned char *dst = out_band + (size_t)yl * A.out_stride + 16u * wx;
                if (!edge) c4_store16(dst, z);
                else c4_store_clip(dst, z, yl < hlim ? (int)wlim - (int)(16u * wx) : 0);
            }
            wave_lds_sync();
            continue;
        }
        // ---- pull my list into registers and sort it by J (network size = the wave's fullest row)
        auto pull_sort = [&](uint32_t (&dd)[16], uint32_t n, bool blank, uint32_t &H, uint32_t &mx) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                uint4 v = make_uint4(0xfffdfffdu, 0xfffdfffdu, 0xfffdfffdu, 0xfffdfffdu);
                if (q < CAP / 8 && (q == 0 || __ballot(n > (uint32_t)(8 * q)) != 0ull)) v = c4_ld16<LSTRIDE>(mylist + 8 * q);
                dd[4 * q + 0] = v.x; dd[4 * q + 1] = v.y; dd[4 * q + 2] = v.z; dd[4 * q + 3] = v.w;
            }
            if (__ballot(blank)) {
                // over-full rows are settled by the direct sum below: their lists must add nothing
#pragma unroll
                for (int q = 0; q < 16; ++q) dd[q] = blank ? 0xfffdfffdu : dd[q];
            }
            if (CAP > 16 && __ballot(n > 16u && !blank) != 0ull) {
                packed_sort<16>(dd); H = 16u;
                mx = __ballot(n > 28u) ? 32u : (__ballot(n > 24u) ? 28u : (__ballot(n > 20u) ? 24u : 20u));
            } else if (CAP > 8 && __ballot(n > 8u && !blank) != 0ull) {
                packed_sort<8>(dd); H = 8u;
                mx = __ballot(n > 12u) ? 16u : 12u;
            } else {
                packed_sort<4>(dd); H = 4u;
                mx = __ballot(n > 4u) ? 8u : 4u;
            }
        };
        bool ovf = cnt > (uint32_t)CAP;
        uint32_t d[16];
        uint32_t Hcur, maxcnt;
        // SPLIT: the crossings left of the strip's middle, when the band was walked in two halves
        [[maybe_unused]] uint32_t dl[SPLIT ? 16 : 1];
        [[maybe_unused]] uint32_t Hl = 0u, maxl = 0u;
        [[maybe_unused]] bool split = false;
        if constexpr (SPLIT) {
            // Over-full rows come in bands (a wiggly outline crosses dozens of neighbouring rows 40 - 60 times): with three
            // or more of them the wave walks the band's pairs twice more, once keeping the crossings of the right half of
            // the sample columns and once those of the left half — 32 slots each, the right half pulled into registers
            // before the left half reuses the lists — and the toggle walk below runs through one after the other (every
            // crossing of the right half lies right of every one of the left).  A row that overflows a half still takes
            // the direct sum.  Three walks instead of one, against ~1 100 vector instructions per over-full row.
#ifdef FR_C4_STATS
            const int n0 = __popcll(__ballot(ovf));
            if (lane == 0) {
                if (n0) { atomicAdd(&g_c4_stats[9], 1ull); atomicAdd(&g_c4_stats[10], (unsigned long long)n0); }   // bands with over-full rows / such rows, first walk
                if (n0 >= 3) { atomicAdd(&g_c4_stats[11], 1ull); atomicAdd(&g_c4_stats[12], (unsigned long long)n0); }   // bands walked in halves / their rows
            }
#endif
            if (__popcll(__ballot(ovf)) >= 3) {
                split = true;
                init_lists();
                eval_pass(NCOL / 2u, NCOL / 2u);             // J in (NCOL / 2, NCOL]
                const uint32_t cr = s_cnt[lane];
                pull_sort(d, cr, cr > (uint32_t)CAP, Hcur, maxcnt);
                wave_lds_sync();
                init_lists();
                eval_pass(0u, NCOL / 2u);                    // J in [1, NCOL / 2]
                const uint32_t cl = s_cnt[lane];
                pull_sort(dl, cl, cl > (uint32_t)CAP, Hl, maxl);
                ovf = (cr > (uint32_t)CAP) | (cl > (uint32_t)CAP);
                if (__ballot(ovf)) {
#pragma unroll
                    for (int q = 0; q < 16; ++q) { d[q] = ovf ? 0xfffdfffdu : d[q]; dl[q] = ovf ? 0xfffdfffdu : dl[q]; }
                }
                cnt = cr + cl;
            }
        }
        if (!split) pull_sort(d, cnt, ovf, Hcur, maxcnt);
        const unsigned long long ovf_rows = __ballot(ovf);
        wave_lds_sync();                        // the list region becomes E below
#ifdef FR_C4_STATS
        // diagnostic build only (make variant NAME=c4stats DEFS=-DFR_C4_STATS): per wave band — sort tier, crossings, over-full rows
        if (lane == 0) {
            atomicAdd(&g_c4_stats[0], 1ull);                                                   // wave bands with crossings
            atomicAdd(&g_c4_stats[Hcur == 4u ? 1 : (Hcur == 8u ? 2 : 3)], 1ull);               // 8- / 16- / 32-slot sort
            atomicAdd(&g_c4_stats[4], (unsigned long long)__popcll(ovf_rows));                 // over-full sample rows
        }
        {
            const uint32_t csum = wave_incl_add(cnt);
            if (lane == 63) atomicAdd(&g_c4_stats[5], (unsigned long long)csum);               // crossings kept (J > 0)
            const unsigned long long g8 = __ballot(cnt > 8u), g16 = __ballot(cnt > 16u), g32 = __ballot(cnt > 32u);
            if (lane == 0) {
                atomicAdd(&g_c4_stats[6], (unsigned long long)__popcll(g8));                   // rows with > 8 / > 16 / > 32 crossings
                atomicAdd(&g_c4_stats[7], (unsigned long long)__popcll(g16));
                atomicAdd(&g_c4_stats[8], (unsigned long long)__popcll(g32));
            }
        }
#endif

        C4_ABL_SORT_ONLY();
        // ---- E: every byte starts at the bias 16
        {
            uint4 *z = reinterpret_cast<uint4 *>(s_E);
            const uint4 bias = make_uint4(0x10101010u, 0x10101010u, 0x10101010u, 0x10101010u);
            constexpr uint32_t NZ = L::E / 16u;
#pragma unroll
            for (uint32_t q = 0; q < (NZ + 63u) / 64u; ++q)
                if (NZ % 64u == 0u || lane + 64u * q < NZ) z[lane + 64u * q] = bias;
        }
        wave_lds_sync();
        // ---- toggles: right to left with the running winding; a crossing that changes zero <-> non-zero adds
        // its two differences to my pixel row's bytes
        if (C4_ABL_KEEP(2)) {
            unsigned char *erow = s_E + (lane >> LN) * L::EROW;
            int run = 0;
            bool zero = true;
            // toggles alternate (zero <-> non-zero), so -sigma of the next toggle is a register that flips:
            // A = 255 * (-sigma), B = NS * (-sigma); V = e0 + 256 e1 = -sigma (255 f + NS) = f A + B
            int A255 = -255, B4 = -NS, ns = -1;
            auto slot = [&](uint32_t dw, int o) {       // crossing (J << 2) | code in bits o .. o + 15 of dw
                run += (int)((dw >> o) & 3u) - 1;
                const bool z = run == 0;
                if (z != zero) {
                    const uint32_t nib = (dw >> (o + 2)) & (uint32_t)(4 * NS - 1);   // (P & 3) << LN | f,  P = J / NS, f = J % NS
                    const int V = __mul24((int)(nib & (uint32_t)(NS - 1)), A255) + B4;
                    const uint32_t sh = (dw >> (o + LN - 1)) & 0x18u;       // 8 (P & 3)
                    uint32_t *dwp = reinterpret_cast<uint32_t *>(erow + ((dw >> (o + LN + 2)) & 0xffcu));
                    atomicAdd(dwp, (uint32_t)V << sh);
                    // the second difference of a pixel in byte 3 belongs to the next dword: e1 = -sigma f
                    // there, 0 elsewhere — f if (P & 3) == 3, i.e. nib - 3 NS saturated at 0
                    const uint32_t g3 = __builtin_elementwise_sub_sat(nib, (uint32_t)(3 * NS));
                    atomicAdd(dwp + 1, (uint32_t)__mul24((int)g3, ns));
                    A255 = -A255; B4 = -B4; ns = -ns;
                }
                zero = z;
            };
            auto walk = [&](const uint32_t (&dd)[16], uint32_t H, uint32_t mx) {
#pragma unroll
                for (int gq = CAP / 8 - 1; gq >= 0; --gq) {
                    if ((uint32_t)(4 * gq) >= H || H + (uint32_t)(4 * gq) >= mx) continue;           // wave-uniform
#pragma unroll
                    for (int j = 4 * gq + 3; j >= 4 * gq; --j) slot(dd[j], 16);
                }
#pragma unroll
                for (int gq = CAP / 8 - 1; gq >= 0; --gq) {
                    if ((uint32_t)(4 * gq) >= H || (uint32_t)(4 * gq) >= mx) continue;               // wave-uniform
#pragma unroll
                    for (int j = 4 * gq + 3; j >= 4 * gq; --j) slot(dd[j], 0);
                }
            };
            walk(d, Hcur, maxcnt);
            if constexpr (SPLIT) { if (split) walk(dl, Hl, maxl); }
            // the row's constant: NS [w(0) != 0], into byte 0 of the pixel row
            if (run != 0) atomicAdd(reinterpret_cast<uint32_t *>(erow), (uint32_t)NS);
        }
        if (__builtin_expect(ovf_rows != 0ull, 0)) {
            // ---- over-full sample rows (more than CAP crossings): the direct sum.  Every record whose row range holds
            // the row is evaluated once more; the winding of every sample column follows from the (J, step) pairs, and
            // lane L turns the non-zero counts of its 16 columns' pixels into E's difference form.
            // Instances that keep 32 crossings (WD != 0): the steps go to a row of 16-bit winding DIFFERENCES in LDS
            // (w(j) = sum over i >= j of d[i]: d[J - 1] += step; the 2 KB next to E, free since the lists were pulled), a
            // suffix sum (16 columns per lane + one wave scan) gives the windings.  Instances that keep <= 16 (WD == 0:
            // glyphs of few crossings per ray — such a row is one in 100 000 there) have no LDS for that row — it is what
            // lets six of their workgroups share a CU — and broadcast every pair to all lanes instead (v_readlane).
            uint32_t *s_wd = reinterpret_cast<uint32_t *>(wregion + L::E);      // [NCOL / 2] x two int16 fields, bias 0x4000
            static_assert(L::WD == 0u || L::WAVE >= L::E + NCOL * 2u, "no room for the winding differences of an over-full row");
            // the reference's evaluation of record k at ray height cy_r -> J (sample columns left of the crossing) and its step
            auto evaluate = [&](uint32_t k, float cy_r, int &J, uint32_t &step) {
                const Rec40 rk = s_rec[k];
                const bool lin = (int32_t)rk.fr < 0;
                const float delta0 = cy_r * rk.a + rk.c1 - rk.c2;
                const float delta = FILL ? __builtin_fmaxf(delta0, 0.0f) : delta0;
                const float num = lin ? (cy_r - rk.b) : (rk.b + sqrt_rn(delta) * rk.sgn);
                const float t = div_by_int(num, rk.a, rk.rden);
                const float xx = (rk.ax * t + rk.bx) * t + rk.p0x;
                const float dy = rk.a * t - rk.b;
                step = ((dy > 0.0f) ? ((rk.fr >> 26) & 3u) : ((rk.fr >> 24) & 3u)) - 1u;   // +1 or -1 (mod 2^32)
                J = (int)__builtin_amdgcn_fmed3f(__builtin_fmaf(xx, jscale, -joff), 0.0f, ncolf);
                const float c0 = s_cxp[J], c1 = s_cxp[J + 1];               // one paired read; the guess is nearly always right
                if (__builtin_expect(!((c0 <= xx) & (xx < c1)), 0)) {
                    while (s_cxp[J + 1] <= xx) ++J;
                    while (s_cxp[J] > xx) --J;
                }
            };
            unsigned long long todo = ovf_rows;
            while (todo) {
                const uint32_t r = (uint32_t)__builtin_ctzll(todo);
                todo &= todo - 1ull;
                const float cy_r = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, cy), (int)r));
                const uint32_t grow = row_b0 + r;
                unsigned long long hm[RPL];
                uint32_t total = 0u;
#pragma unroll
                for (int i = 0; i < RPL; ++i) {
                    hm[i] = __ballot(rra[i] <= grow && grow < rre[i]);      // the rows that accept this root (exact)
                    total += (uint32_t)__popcll(hm[i]);
                }
                int wcol[16];                                               // the winding at my 16 sample columns
                if constexpr (L::WD != 0u) {
                    for (uint32_t q = lane; q < NCOL * 2u / 16u; q += 64u)
                        reinterpret_cast<uint4 *>(s_wd)[q] = make_uint4(0x40004000u, 0x40004000u, 0x40004000u, 0x40004000u);
                    wave_lds_sync();
                    auto add = [&](uint32_t k) {
                        int J; uint32_t step;
                        evaluate(k, cy_r, J, step);
                        if (J > 0) atomicAdd(&s_wd[(uint32_t)(J - 1) >> 1], step << (16u * ((uint32_t)(J - 1) & 1u)));
                    };
                    // The records that hold the row are a few dozen of up to 64 RPL, scattered over the lanes' RPL slots:
                    // walking the slots would run RPL divergent evaluations at a few per cent of the lanes each.  Instead
                    // every hit is pushed to a dense lane first (ds_permute: a forward permutation, no LDS memory) — slot
                    // i's hits go to the dense positions fill .. fill + c - 1, its other lanes fill the rest of the same
                    // permutation — and the evaluation runs once per 64 hits.
                    if (__builtin_expect(total <= 128u, 1)) {
                        uint32_t fill = 0u;                                 // dense positions in use
                        uint32_t kd0 = 0xffffffffu, kd1 = 0xffffffffu;      // my dense record index: positions 0 .. 63 / 64 .. 127
#pragma unroll
                        for (int i = 0; i < RPL; ++i) {
                            if (hm[i] == 0ull) continue;                    // (wave-uniform)
                            const bool hit = (hm[i] >> lane) & 1ull;
                            const uint32_t c = (uint32_t)__popcll(hm[i]);
                            const uint32_t below = __builtin_amdgcn_mbcnt_hi((uint32_t)(hm[i] >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)hm[i], 0u));
                            // hits -> dense positions fill + rank (lane = position mod 64), the other lanes -> the lanes left over
                            const uint32_t dst = hit ? ((fill + below) & 63u) : ((fill + c + (lane - below)) & 63u);
                            const uint32_t got = (uint32_t)__builtin_amdgcn_ds_permute((int)(dst << 2), (int)(hit ? per * lane + (uint32_t)i : 0xffffffffu));
                            const uint32_t end = fill + c;
                            kd0 = (lane >= fill && lane < end) ? got : kd0;
                            kd1 = (lane + 64u >= fill && lane + 64u < end) ? got : kd1;
                            fill = end;
                        }
                        if (kd0 != 0xffffffffu) add(kd0);
                        if (fill > 64u) { if (kd1 != 0xffffffffu) add(kd1); }
                    } else {
                        // (more than 128 records hold the row: slot by slot, as they sit)
#pragma unroll
                        for (int i = 0; i < RPL; ++i)
                            if ((hm[i] >> lane) & 1ull) add(per * lane + (uint32_t)i);
                    }
                    wave_lds_sync();
                    int tot = 0;
                    if (16u * lane < NCOL) {
                        const uint4 lo4 = reinterpret_cast<const uint4 *>(s_wd)[2u * lane], hi4 = reinterpret_cast<const uint4 *>(s_wd)[2u * lane + 1u];
                        const uint32_t dws[8] = {lo4.x, lo4.y, lo4.z, lo4.w, hi4.x, hi4.y, hi4.z, hi4.w};
#pragma unroll
                        for (int c = 15; c >= 0; --c) {
                            tot += (int)((dws[c >> 1] >> (16 * (c & 1))) & 0xffffu) - 0x4000;
                            wcol[c] = tot;                                  // columns c .. 15 of my 16
                        }
                    } else {
#pragma unroll
                        for (int c = 0; c < 16; ++c) wcol[c] = 0;
                    }
                    const uint32_t incl = wave_incl_add((uint32_t)tot);
                    const int right = (int)((uint32_t)__builtin_amdgcn_readlane((int)incl, 63) - incl);   // everything right of my 16 columns
#pragma unroll
                    for (int c = 0; c < 16; ++c) wcol[c] += right;
                } else {
#pragma unroll
                    for (int c = 0; c < 16; ++c) wcol[c] = 0;
                    const int col0 = (int)(16u * lane);                     // my first sample column
#pragma unroll
                    for (int i = 0; i < RPL; ++i) {
                        if (hm[i] == 0ull) continue;                        // (wave-uniform)
                        int J = 0; uint32_t step = 0u;
                        if ((hm[i] >> lane) & 1ull) evaluate(per * lane + (uint32_t)i, cy_r, J, step);
                        unsigned long long m = hm[i];
                        while (m) {                                         // every crossing to every lane: w(j) += step [j < J]
                            const int h = (int)__builtin_ctzll(m);
                            m &= m - 1ull;
                            const int n = __builtin_amdgcn_readlane(J, h) - col0;
                            const int sh = __builtin_amdgcn_readlane((int)step, h);
#pragma unroll
                            for (int c = 0; c < 16; ++c) wcol[c] += (c < n) ? sh : 0;
                        }
                    }
                }
                constexpr int PPL = 16 / NS;                              // pixels of my 16 sample columns
                int cq[PPL];
#pragma unroll
                for (int q = 0; q < PPL; ++q) {
                    cq[q] = 0;
#pragma unroll
                    for (int c = 0; c < NS; ++c) cq[q] += (wcol[NS * q + c] != 0);
                }
                int prev = __shfl_up(cq[PPL - 1], 1);
                if (lane == 0) prev = 0;
#pragma unroll
                for (int dq = 0; dq < PPL / 4; ++dq) {
                    const int before = dq ? cq[4 * dq - 1] : prev;
                    const uint32_t val = (uint32_t)(cq[4 * dq] - before) + ((uint32_t)(cq[4 * dq + 1] - cq[4 * dq]) << 8) +
                                         ((uint32_t)(cq[4 * dq + 2] - cq[4 * dq + 1]) << 16) + ((uint32_t)(cq[4 * dq + 3] - cq[4 * dq + 2]) << 24);
                    if (16u * lane < NCOL) atomicAdd(reinterpret_cast<uint32_t *>(s_E + (r >> LN) * L::EROW) + lane * (uint32_t)(PPL / 4) + (uint32_t)dq, val);
                }
                wave_lds_sync();
            }
        }
        wave_lds_sync();

        // ---- windows: lane = one 16-pixel window of one pixel row; integrate, map, one 16-byte store
        constexpr uint32_t K1 = 0x01010101u;
        // (one window pass: the hot form stores whole windows; a band or strip cut by the cell's border runs the same
        // arithmetic in a loop of its own — rolled, clipped stores — so that the hot loop stays as small as it was)
        // (The window addresses depend on the lane only, so the compiler computes them once per kernel, keeps them live across
        // the band loop and — in the 80-register instances — spills them; every reload is then a scratch load, and on gfx9 a
        // wave waits for a load with s_waitcnt vmcnt(0), which also waits for every pixel store it still has in flight: a band's
        // stores went out one HBM round trip at a time.  An opaque copy of the lane per band keeps the addresses where they
        // are used — a few integer instructions per window instead; and the store address is a 32-bit offset from the band's
        // wave-uniform base: PRB rows of < 2^27 bytes, fr_plan_render checks the pitch.)
        uint32_t lane_w = lane;
        asm volatile("" : "+v"(lane_w));
        const uint32_t wxw = lane_w & (NWIN - 1u);
        // (my window of pass 0, in E and in the output; pass `it` is 64 >> WLOG rows further down: a constant / a scalar away)
        const unsigned char *const e_lane = s_E + (lane_w >> WLOG) * L::EROW + 16u * wxw;
        const uint32_t out_lane = (lane_w >> WLOG) * (uint32_t)A.out_stride + 16u * wxw;
        auto window_pass = [&](uint32_t it, auto clipped) {
            const uint32_t prow = (lane_w >> WLOG) + it * (64u >> WLOG);
            const uint4 e = *reinterpret_cast<const uint4 *>(e_lane + it * (64u >> WLOG) * L::EROW);
            // inclusive byte prefix inside each dword: bytes 16 (i + 1) + sums; back to a bias of 16 per byte
            uint32_t x0 = e.x * K1, x1 = e.y * K1, x2 = e.z * K1, x3 = e.w * K1;
            x0 -= 0x30201000u;
            x1 = x1 + __builtin_amdgcn_perm(x0, x0, 0x03030303u) - 0x40302010u;
            x2 = x2 + __builtin_amdgcn_perm(x1, x1, 0x03030303u) - 0x40302010u;
            x3 = x3 + __builtin_amdgcn_perm(x2, x2, 0x03030303u) - 0x40302010u;
            // count entering my window = sum of the windows to my left in the pixel row
            const uint32_t T = (x3 >> 24) - 16u;                            // my window's total (signed)
            uint32_t inc = T;
            if (WLOG == 4) {
                inc += dpp<0x111>(inc);                                 // row_shr:1 within the 16 lanes of my pixel row
                inc += dpp<0x112>(inc);
                inc += dpp<0x114>(inc);
                inc += dpp<0x118>(inc);
            } else {
                // 8 (4) windows per pixel row: two (four) pixel rows share a DPP row — keep the scan inside each part
                uint32_t s;
                s = dpp<0x111>(inc); inc += (wxw >= 1u) ? s : 0u;
                s = dpp<0x112>(inc); inc += (wxw >= 2u) ? s : 0u;
                if (WLOG == 3) { s = dpp<0x114>(inc); inc += (wxw >= 4u) ? s : 0u; }
            }
            const uint32_t cin = inc - T;                                   // in [0, NS^2]
            const uint32_t cb4 = __builtin_amdgcn_perm(cin, cin, 0x00000000u);
            x0 += cb4; x1 += cb4; x2 += cb4; x3 += cb4;                     // bytes: 16 + k, k = inside samples of the pixel
            // u8 = round_half_up(255 k / NS^2) = 16 k - [k > 8] (NS = 4) / 64 k - [k > 2] (NS = 2), four pixels at once:
            // (16 + k) << s leaves 2^(4 + s) too much in every byte — 0x01010100 (0x04040400) over the dword, mod 2^32
            auto map4 = [](uint32_t x) -> uint32_t {
                uint32_t r;
                if (NS == 4) {
                    const uint32_t t = ((x + 0x07070707u) >> 5) & 0x01010101u;
                    const uint32_t u = 0xfefeff00u - t;
                    asm("v_lshl_add_u32 %0, %1, 4, %2" : "=v"(r) : "v"(x), "v"(u));      // (x << 4) + u in one instruction
                } else {
                    const uint32_t t = ((x + 0x0d0d0d0du) >> 5) & 0x01010101u;
                    const uint32_t u = 0xfbfbfc00u - t;
                    asm("v_lshl_add_u32 %0, %1, 6, %2" : "=v"(r) : "v"(x), "v"(u));
                }
                return r;
            };
            const uint4 v = make_uint4(map4(x0), map4(x1), map4(x2), map4(x3));
            unsigned char *dst = (out_band + (size_t)(it * (64u >> WLOG)) * A.out_stride) + out_lane;
            if (!decltype(clipped)::value) c4_store16(dst, v);
            else c4_store_clip(dst, v, prow < hlim ? (int)wlim - (int)(16u * wxw) : 0);
        };
        if (C4_ABL_KEEP(1)) {
            if (__builtin_expect(!edge, 1)) {
#pragma unroll
                for (uint32_t it = 0; it < (PRB * NWIN) / 64u; ++it) window_pass(it, std::false_type{});
            } else {
#pragma clang loop unroll(disable)
                for (uint32_t it = 0; it < (PRB * NWIN) / 64u; ++it) window_pass(it, std::true_type{});
            }
        }
        wave_lds_sync();                        // E is the next band's list region
    }

// fr_text_colour_kernel.inc — the rows of one tile as RGBA pixels: the body of colour_rows and of text_rgba_load_kernel
// (fr_text.hip, which describes it), and of affine_colour_rows (fr_text_affine.hip).  Uses INST, N, FILL, BLEND, SRGB, LOAD, PLACE, a.
// With FR_TEXT_MASK_CACHED defined (fr_text_cached.hip only) the masks are loaded from a.masks: see fr_text_cover_kernel.inc.
    constexpr uint32_t NN = (uint32_t)(N * N);
    constexpr uint32_t FULL = NN == 32u ? ~0u : (1u << NN) - 1u;
    constexpr uint32_t LG = N == 4 ? 4u : N == 2 ? 2u : 0u;              // log2(n^2)
    constexpr uint32_t M2 = 0x00ff00ffu;
    [[maybe_unused]] const uint16_t *D = nullptr, *K = nullptr;
    if constexpr (SRGB) {
        __shared__ uint4 lds_d[sizeof SRGB_D / 16], lds_k[sizeof SRGB_K / 16];
        for (uint32_t i = threadIdx.x; i < sizeof SRGB_K / 16; i += 64 * TEXT_WAVES)
            lds_k[i] = reinterpret_cast<const uint4 *>(SRGB_K)[i];
        if (threadIdx.x < sizeof SRGB_D / 16) lds_d[threadIdx.x] = reinterpret_cast<const uint4 *>(SRGB_D)[threadIdx.x];
        __syncthreads();
        D = reinterpret_cast<const uint16_t *>(lds_d);
        K = reinterpret_cast<const uint16_t *>(lds_k);
    }
    const TextTile tl = a.tiles[blockIdx.x];
    const TextRun rn = a.runs[tl.run];
    const int lane = (int)(threadIdx.x & 63u);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int X = (int)tl.x0 + lane;
    float off[N];
#pragma unroll
    for (int k = 0; k < N; ++k) off[k] = sub_off(k, N, a.phase_center);
    for (int yy = wave; yy < TEXT_TILE_H; yy += TEXT_WAVES) {
        const int Y = (int)tl.y0 + yy;
        if (Y >= (int)rn.h) break;
        uint32_t *px = reinterpret_cast<uint32_t *>(a.out) + ((uint64_t)rn.out_y + (uint64_t)Y) * a.out_stride + rn.out_x + (uint32_t)X;
        uint32_t start = rn.clear;                                         // what every sample holds before the first instance
        if constexpr (LOAD) start = X < (int)rn.w ? *px : 0u;             // (X < w, Y < h: the store's guard)
        // channel sums.  RGBA: c0 = R | B << 16, c1 = G | A << 16.  sRGB: linear R, G, B (<= 16 * 65535) and alpha
        uint32_t c0 = 0u, c1 = 0u, c2 = 0u, c3 = 0u;
        bool keep = false;                                                 // (LOAD) every sample untaken: the pixel stays
        if constexpr (BLEND == 0) {
            uint32_t taken = 0u;
            for (uint32_t q = tl.lend; q > tl.lbeg;) {
                const INST in = a.insts[a.list[--q]];
                if (Y < in.y0 || Y >= in.y1) continue;                   // (wave-uniform)
                const bool inside = X >= in.x0 && X < in.x1;
                uint32_t m;
#ifdef FR_TEXT_MASK_CACHED
                m = 0u;
                if (inside) m = a.masks[in.base + (uint32_t)(Y - in.r0) * in.pitch + (uint32_t)(X - in.c0)];
#else
                if constexpr (std::is_same_v<INST, TextInstAffine>) {
#include "fr_text_affine_mask_kernel.inc"
                } else {
#include "fr_text_mask_kernel.inc"
                }
#endif
                if (inside) {
                    const uint32_t k = (uint32_t)__builtin_popcount(m & ~taken);
                    if constexpr (SRGB) {
                        c0 += k * (in.pad[0] & 0xffffu);
                        c1 += k * (in.pad[0] >> 16);
                        c2 += k * in.pad[1];
                        c3 += k * (in.rgba >> 24);
                    } else {
                        c0 += k * (in.rgba & M2);
                        c1 += k * ((in.rgba >> 8) & M2);
                    }
                    taken |= m;
                }
            }
            const uint32_t k = (uint32_t)__builtin_popcount(~taken & FULL);
            if constexpr (SRGB && LOAD) {
                c0 += k * D[start & 0xffu];
                c1 += k * D[(start >> 8) & 0xffu];
                c2 += k * D[(start >> 16) & 0xffu];
                c3 += k * (start >> 24);
            } else if constexpr (SRGB) {
                c0 += k * (rn.pad[0] & 0xffffu);
                c1 += k * (rn.pad[0] >> 16);
                c2 += k * rn.pad[1];
                c3 += k * (start >> 24);
            } else {
                c0 += k * (start & M2);
                c1 += k * ((start >> 8) & M2);
            }
            keep = LOAD && FR_TEXT_LOAD_SKIP && taken == 0u;
        } else {
            uint32_t smp[NN];
#pragma unroll
            for (uint32_t k = 0; k < NN; ++k) smp[k] = start;
            for (uint32_t q = tl.lbeg; q < tl.lend; ++q) {
                const INST in = a.insts[a.list[q]];
                if (Y < in.y0 || Y >= in.y1) continue;                   // (wave-uniform)
                const bool inside = X >= in.x0 && X < in.x1;
                uint32_t m;
#ifdef FR_TEXT_MASK_CACHED
                m = 0u;
                if (inside) m = a.masks[in.base + (uint32_t)(Y - in.r0) * in.pitch + (uint32_t)(X - in.c0)];
#else
                if constexpr (std::is_same_v<INST, TextInstAffine>) {
#include "fr_text_affine_mask_kernel.inc"
                } else {
#include "fr_text_mask_kernel.inc"
                }
#endif
                const uint32_t hit = inside ? m : 0u;
                const uint32_t A = in.rgba >> 24, ia = 255u - A, hiA = in.rgba & 0xff000000u;
                if constexpr (SRGB) {
                    const uint32_t rA = (in.pad[0] & 0xffffu) * A + 127u, gA = (in.pad[0] >> 16) * A + 127u, bA = in.pad[1] * A + 127u;
                    [[maybe_unused]] const uint32_t aA = 255u * A + 127u;                  // (BLEND = 2) alpha: the colour formula with C = 255, linear
#pragma unroll
                    for (uint32_t k = 0; k < NN; ++k) {
                        if (hit >> k & 1u) {
                            const uint32_t sm = smp[k];
                            const uint32_t r = srgb_encode(K, div255_24(rA + (uint32_t)D[sm & 0xffu] * ia));
                            const uint32_t g = srgb_encode(K, div255_24(gA + (uint32_t)D[(sm >> 8) & 0xffu] * ia));
                            const uint32_t b = srgb_encode(K, div255_24(bA + (uint32_t)D[(sm >> 16) & 0xffu] * ia));
                            if constexpr (BLEND == 2) smp[k] = r | g << 8 | b << 16 | div255_24(aA + (sm >> 24) * ia) << 24;
                            else smp[k] = r | g << 8 | b << 16 | hiA;
                        }
                    }
                } else {
                    const uint32_t rbA = (in.rgba & M2) * A + 0x00800080u, gA = ((in.rgba >> 8) & 0xffu) * A + 128u;
                    // (BLEND = 2) the sample's alpha rides the high half of the G call, its source 255: G | a << 16
                    [[maybe_unused]] const uint32_t gaA = (((in.rgba >> 8) & 0xffu) | 255u << 16) * A + 0x00800080u;
#pragma unroll
                    for (uint32_t k = 0; k < NN; ++k) {
                        if constexpr (BLEND == 2) {
                            if (hit >> k & 1u) smp[k] = blend2(smp[k] & M2, rbA, ia) | (blend2((smp[k] >> 8) & M2, gaA, ia) << 8);
                        } else {
                            if (hit >> k & 1u)
                                smp[k] = blend2(smp[k] & M2, rbA, ia) | (blend2((smp[k] >> 8) & 0xffu, gA, ia) << 8) | hiA;
                        }
                    }
                }
            }
#pragma unroll
            for (uint32_t k = 0; k < NN; ++k) {
                if constexpr (SRGB) {
                    c0 += D[smp[k] & 0xffu];
                    c1 += D[(smp[k] >> 8) & 0xffu];
                    c2 += D[(smp[k] >> 16) & 0xffu];
                    c3 += smp[k] >> 24;
                } else {
                    c0 += smp[k] & M2;                                     // at most 16 * 255 per half
                    c1 += (smp[k] >> 8) & M2;
                }
            }
        }
        if (X < (int)rn.w && !keep) {
            uint32_t v;
            if constexpr (SRGB) {
                constexpr uint32_t HALF = NN / 2u;
                v = srgb_encode(K, (c0 + HALF) >> LG) | srgb_encode(K, (c1 + HALF) >> LG) << 8 |
                    srgb_encode(K, (c2 + HALF) >> LG) << 16 | ((c3 + HALF) >> LG) << 24;
            } else {
                constexpr uint32_t HALF = (NN / 2u) * 0x00010001u;
                v = (((c0 + HALF) >> LG) & M2) | ((((c1 + HALF) >> LG) & M2) << 8);
            }
            __builtin_nontemporal_store(v, px);
        }
    }

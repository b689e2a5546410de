// fr_text_cover_kernel.inc — the rows of one tile as coverage / mask bytes: the body of text_kernel and text_place_kernel
// (fr_text.hip) and of text_affine_kernel (fr_text_affine.hip).  Uses INST, N, FILL, PLACE, a.  Text, not a function: see the note on the instances in fr_text.hip.
// With FR_TEXT_MASK_CACHED defined (fr_text_cached.hip only: a preprocessor switch, so that the other units see the text they had)
// the instance's mask is loaded from its key's cell in a.masks instead of being evaluated.
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
        uint32_t mask = 0u;
        for (uint32_t q = tl.lbeg; q < tl.lend; ++q) {
            const INST in = a.insts[a.list[q]];
            if (Y < in.y0 || Y >= in.y1) continue;                       // (wave-uniform)
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
            if (inside) mask |= m;
        }
        if (X < (int)rn.w) {                                               // every pixel of the run: 0 where no instance reaches
            constexpr uint32_t NN = (uint32_t)(N * N);
            const uint8_t v = (uint8_t)((510u * (uint32_t)__builtin_popcount(mask) + NN) / (2u * NN));    // round_half_up(255 k / n^2)
            uint8_t *dst = a.out + ((uint64_t)rn.out_y + (uint64_t)Y) * a.out_stride + rn.out_x + (uint32_t)X;
            __builtin_nontemporal_store(v, dst);
        }
    }

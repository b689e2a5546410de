// fr_layer_outline_plan.cpp — the host side of fr_layer_outline (fr_layer_outline_plan.hpp).  No HIP.
#include "fr_layer_outline_plan.hpp"

#include <algorithm>
#include <cmath>

namespace fr {

int set_error(int code, const char *fmt, ...);         // the context unit (the self-test has its own)

static int check_image(const char *what, uintptr_t p, size_t stride)
{
    if (!p) return set_error(FR_E_INVALID, "%s is NULL", what);
    if (p & 3u) return set_error(FR_E_INVALID, "%s %p is not 4-byte aligned", what, (void *)p);
    if (stride > ((size_t)1 << 26)) return set_error(FR_E_INVALID, "%s: row pitch of %zu elements: at most 2^26", what, stride);
    return FR_OK;
}

// floor(sqrt(n)), n < 2^31: the double's root is within one of it
static uint32_t isqrt(uint32_t n)
{
    uint32_t q = (uint32_t)std::sqrt((double)n);
    while ((uint64_t)q * q > n) --q;
    while ((uint64_t)(q + 1) * (q + 1) <= n) ++q;
    return q;
}

uint32_t outline_weight(uint32_t rho, int32_t i, int32_t j)
{
    const int32_t q = (int32_t)isqrt(65536u * (uint32_t)(i * i + j * j));     // |i|, |j| <= 16: below 2^25
    const int32_t t = 16 * (int32_t)rho + 256 - q;
    return t <= 0 ? 0u : (uint32_t)std::min(255, (255 * t + 128) / 256);
}

void outline_table(uint32_t rho, OutlineTable &out)
{
    out = OutlineTable{};
    const int32_t R = (int32_t)outline_reach(rho), R4 = (int32_t)outline_reach4(rho), n = 2 * R + 1;
    const uint32_t nw = outline_row_words(rho);
    out.reach = (uint32_t)R;
    out.reach4 = (uint32_t)R4;
    out.row_words = nw;
    out.k.resize((size_t)n * n);
    out.rows.resize((size_t)n);
    const size_t weights_at = 4 * (size_t)n;                    // one unit per row
    out.packed.assign((weights_at + (size_t)n * nw + 3) / 4 * 4, 0u);
    for (int32_t j = -R; j <= R; ++j) {
        OutlineRow &row = out.rows[(size_t)(j + R)];
        row = OutlineRow{-1, 0u, 0u, 0u};
        for (int32_t i = -R; i <= R; ++i) {
            const uint32_t k = outline_weight(rho, i, j);
            out.k[(size_t)(j + R) * n + (i + R)] = (uint8_t)k;
            if (!k) continue;
            if (k == 255u) row.core = std::max(row.core, i);
            else if (i >= 0) ++row.rim;
            const uint32_t t = (uint32_t)(i + R4);
            out.packed[weights_at + (size_t)(j + R) * nw + t / 4] |= k << (8 * (t % 4));
        }
        while (row.core >= 0 && (2u << row.level) <= 2u * (uint32_t)row.core + 1u) ++row.level;
        out.levels = std::max(out.levels, row.level);
        const uint32_t head[4] = {(uint32_t)row.core, row.rim, row.level, 0u};
        std::copy(head, head + 4, out.packed.begin() + 4 * (j + R));
    }
}

static ShadowRect grow(const ShadowRect &r, int64_t by) { return ShadowRect{r.x0 - by, r.y0 - by, r.x1 + by, r.y1 + by}; }

static ShadowRect cut(const ShadowRect &a, const ShadowRect &b)
{
    const ShadowRect r{std::max(a.x0, b.x0), std::max(a.y0, b.y0), std::min(a.x1, b.x1), std::min(a.y1, b.y1)};
    return r.empty() ? ShadowRect{0, 0, 0, 0} : r;
}

int outline_plan(const OutlineIn &in, OutlinePlan &out)
{
    out = OutlinePlan{};
    if (in.flags & ~(uint32_t)FR_LAYER_SRGB) return set_error(FR_E_INVALID, "unknown flag bits 0x%x", in.flags & ~(uint32_t)FR_LAYER_SRGB);
    if (const int rc = check_image("src", in.src, in.src_stride)) return rc;
    if (const int rc = check_image("dst", in.dst, in.dst_stride)) return rc;
    if (in.src_rows > SHADOW_MAX_ROWS || in.dst_rows > SHADOW_MAX_ROWS) return set_error(FR_E_UNSUPPORTED, "an image of more than 2^31 - 1 rows");
    if (!in.outline) return set_error(FR_E_INVALID, "outline is NULL");
    const fr_layer_outline_params &s = *in.outline;
    const bool window = s.w && s.h, rect = s.dst_w && s.dst_h;
    if (window && ((uint64_t)s.src_x + s.w > in.src_stride || (uint64_t)s.src_y + s.h > in.src_rows))
        return set_error(FR_E_INVALID, "outline: the window of %u x %u at (%u, %u) leaves the layer of %zu x %zu", s.w, s.h, s.src_x, s.src_y,
                         in.src_stride, in.src_rows);
    if (rect && ((uint64_t)s.dst_x + s.dst_w > in.dst_stride || (uint64_t)s.dst_y + s.dst_h > in.dst_rows))
        return set_error(FR_E_INVALID, "outline: the rectangle of %u x %u at (%u, %u) leaves the destination of %zu x %zu", s.dst_w, s.dst_h,
                         s.dst_x, s.dst_y, in.dst_stride, in.dst_rows);
    if (s.radius > FR_OUTLINE_MAX_RADIUS) return set_error(FR_E_INVALID, "outline: radius %u above 256 (16 pixels)", s.radius);
    if (s.kind > FR_OUTLINE_SHRINK) return set_error(FR_E_INVALID, "outline: kind %u is none of FR_OUTLINE_*", s.kind);
    // the two images' bytes (stride <= 2^26, rows < 2^31: no overflow)
    const uintptr_t src_end = in.src + 4 * in.src_stride * in.src_rows, dst_end = in.dst + 4 * in.dst_stride * in.dst_rows;
    if (in.src < dst_end && in.dst < src_end) return set_error(FR_E_INVALID, "the layer and the destination overlap in memory");

    if (rect && ((uint64_t)s.dst_w + 3 + SHADOW_TILE - 1) / SHADOW_TILE * (((uint64_t)s.dst_h + SHADOW_TILE - 1) / SHADOW_TILE) > SHADOW_MAX_TILES)
        return set_error(FR_E_UNSUPPORTED, "outline: the rectangle of %u x %u needs more than 2^22 tiles; split the call", s.dst_w, s.dst_h);

    out.nothing = !rect;
    out.want = ShadowRect{-(int64_t)s.dx, -(int64_t)s.dy, -(int64_t)s.dx + s.dst_w, -(int64_t)s.dy + s.dst_h};
    if (!rect) return FR_OK;
    out.vec = in.dst_stride % 4 == 0;
    out.lead = out.vec ? (uint32_t)(((in.dst >> 2) + (uint64_t)s.dst_y * in.dst_stride + s.dst_x) & 3u) : 0u;
    out.tiles_x = ((uint64_t)s.dst_w + out.lead + SHADOW_TILE - 1) / SHADOW_TILE;
    out.tiles_y = ((uint64_t)s.dst_h + SHADOW_TILE - 1) / SHADOW_TILE;
    const bool outward = s.kind == FR_OUTLINE_GROW || s.kind == FR_OUTLINE_RING;
    const ShadowRect win{0, 0, (int64_t)s.w, (int64_t)s.h};
    if (window) out.live = cut(out.want, outward ? grow(win, outline_reach(s.radius)) : win);
    // at radius 0 the weight is K(0, 0) = 255 alone: G[A] = A and S = A0, so RING and INNER are zero
    if (out.live.empty() || (s.radius == 0 && (s.kind == FR_OUTLINE_RING || s.kind == FR_OUTLINE_INNER))) {
        out.live = ShadowRect{0, 0, 0, 0};
        out.zeros = true;
        return FR_OK;
    }
    outline_table(s.radius, out.table);
    return FR_OK;
}

}  // namespace fr

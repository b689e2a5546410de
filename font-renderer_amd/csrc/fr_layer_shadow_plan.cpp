// fr_layer_shadow_plan.cpp — the host side of fr_layer_shadow (fr_layer_shadow_plan.hpp).  No HIP.
#include "fr_layer_shadow_plan.hpp"

#include <algorithm>

namespace fr {

int set_error(int code, const char *fmt, ...);         // the context unit (the self-test has its own)

static int check_image(const char *what, uintptr_t p, size_t stride)
{
    if (!p) return set_error(FR_E_INVALID, "%s is NULL", what);
    if (p & 3u) return set_error(FR_E_INVALID, "%s %p is not 4-byte aligned", what, (void *)p);
    if (stride > ((size_t)1 << 26)) return set_error(FR_E_INVALID, "%s: row pitch of %zu elements: at most 2^26", what, stride);
    return FR_OK;
}

ShadowRecip shadow_recip(uint32_t radius)
{
    const uint64_t W = (uint64_t)(2 * radius + 1) * (2 * radius + 1);
    uint32_t shift = 0;
    while ((W >> (shift + 1)) != 0) ++shift;
    return ShadowRecip{(uint32_t)((((uint64_t)1 << (32 + shift)) + W - 1) / W), shift};
}

static ShadowRect grow(const ShadowRect &r, int64_t by) { return ShadowRect{r.x0 - by, r.y0 - by, r.x1 + by, r.y1 + by}; }

static ShadowRect cut(const ShadowRect &a, const ShadowRect &b)
{
    const ShadowRect r{std::max(a.x0, b.x0), std::max(a.y0, b.y0), std::min(a.x1, b.x1), std::min(a.y1, b.y1)};
    return r.empty() ? ShadowRect{0, 0, 0, 0} : r;
}

int shadow_plan(const ShadowIn &in, ShadowPlan &out)
{
    out = ShadowPlan{};
    if (in.flags & ~(uint32_t)FR_LAYER_SRGB) return set_error(FR_E_INVALID, "unknown flag bits 0x%x", in.flags & ~(uint32_t)FR_LAYER_SRGB);
    if (const int rc = check_image("src", in.src, in.src_stride)) return rc;
    if (const int rc = check_image("dst", in.dst, in.dst_stride)) return rc;
    if (in.src_rows > SHADOW_MAX_ROWS || in.dst_rows > SHADOW_MAX_ROWS) return set_error(FR_E_UNSUPPORTED, "an image of more than 2^31 - 1 rows");
    if (!in.shadow) return set_error(FR_E_INVALID, "shadow is NULL");
    const fr_layer_shadow_params &s = *in.shadow;
    const bool window = s.w && s.h, rect = s.dst_w && s.dst_h;
    if (window && ((uint64_t)s.src_x + s.w > in.src_stride || (uint64_t)s.src_y + s.h > in.src_rows))
        return set_error(FR_E_INVALID, "shadow: the window of %u x %u at (%u, %u) leaves the layer of %zu x %zu", s.w, s.h, s.src_x, s.src_y,
                         in.src_stride, in.src_rows);
    if (rect && ((uint64_t)s.dst_x + s.dst_w > in.dst_stride || (uint64_t)s.dst_y + s.dst_h > in.dst_rows))
        return set_error(FR_E_INVALID, "shadow: the rectangle of %u x %u at (%u, %u) leaves the destination of %zu x %zu", s.dst_w, s.dst_h,
                         s.dst_x, s.dst_y, in.dst_stride, in.dst_rows);
    if (s.spread > SHADOW_MAX_SPREAD) return set_error(FR_E_INVALID, "shadow: spread %u above 8", s.spread);
    if (s.blur_radius > SHADOW_MAX_RADIUS) return set_error(FR_E_INVALID, "shadow: blur_radius %u above 32", s.blur_radius);
    if (s.blur_passes > SHADOW_MAX_PASSES) return set_error(FR_E_INVALID, "shadow: blur_passes %u above 3", s.blur_passes);
    // the two images' bytes (stride <= 2^26, rows < 2^31: no overflow)
    const uintptr_t src_end = in.src + 4 * in.src_stride * in.src_rows, dst_end = in.dst + 4 * in.dst_stride * in.dst_rows;
    if (in.src < dst_end && in.dst < src_end) return set_error(FR_E_INVALID, "the layer and the destination overlap in memory");

    if (rect && ((uint64_t)s.dst_w + 3 + SHADOW_TILE - 1) / SHADOW_TILE * (((uint64_t)s.dst_h + SHADOW_TILE - 1) / SHADOW_TILE) > SHADOW_MAX_TILES)
        return set_error(FR_E_UNSUPPORTED, "shadow: the rectangle of %u x %u needs more than 2^22 tiles; split the call", s.dst_w, s.dst_h);

    out.nothing = !rect;
    out.want = ShadowRect{-(int64_t)s.dx, -(int64_t)s.dy, -(int64_t)s.dx + s.dst_w, -(int64_t)s.dy + s.dst_h};
    if (!rect) return FR_OK;
    std::vector<uint32_t> radii;
    if (s.spread) radii.push_back(s.spread);
    if (s.blur_radius)
        for (uint32_t k = 0; k < s.blur_passes; ++k) radii.push_back(s.blur_radius);
    int64_t reach = 0;
    for (uint32_t r : radii) reach += r;
    const ShadowRect win{0, 0, (int64_t)s.w, (int64_t)s.h};
    if (!window || cut(out.want, grow(win, reach)).empty()) {
        out.zeros = true;
        return FR_OK;
    }
    int64_t before = 0;
    for (size_t k = 0; k < radii.size(); ++k) {
        before += radii[k];
        ShadowStage st{};
        st.kind = k == 0 && s.spread ? SHADOW_SPREAD : SHADOW_BOX;
        st.radius = radii[k];
        st.out = cut(grow(out.want, reach - before), grow(win, before));      // not empty: the want and the window are `reach` apart at most
        if (st.kind == SHADOW_BOX) st.recip = shadow_recip(st.radius);
        if (k + 1 < radii.size()) {
            st.pitch = (st.out.w() + SHADOW_TILE - 1) / SHADOW_TILE * SHADOW_TILE;
            out.plane_bytes[k & 1] = std::max(out.plane_bytes[k & 1], st.pitch * st.out.h());
        }
        out.stages.push_back(st);
    }
    if (out.plane_bytes[0] + out.plane_bytes[1] > SHADOW_MAX_PLANE_BYTES)
        return set_error(FR_E_UNSUPPORTED, "shadow: intermediate planes of %llu bytes: at most 2^30; split the rectangle",
                         (unsigned long long)(out.plane_bytes[0] + out.plane_bytes[1]));
    return FR_OK;
}

}  // namespace fr

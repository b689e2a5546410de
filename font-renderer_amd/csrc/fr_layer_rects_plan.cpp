// fr_layer_rects_plan.cpp — the host side of fr_layer_rects (fr_layer_rects_plan.hpp).  No HIP.
#include "fr_layer_rects_plan.hpp"

#include <algorithm>

namespace fr {

namespace {

constexpr int TILE_X_SHIFT = 14, TILE_Y_SHIFT = 10;    // 1/64 pixel -> tile column / tile row
static_assert((64u * LAYER_TILE_W) == (1u << TILE_X_SHIFT) && (64u * LAYER_TILE_H) == (1u << TILE_Y_SHIFT), "tile shifts");
// a (tile, record) pair as one sortable word: tile row (21 bits), tile column (17 bits), record (24 bits)
constexpr int KEY_X_BITS = 17, KEY_REC_BITS = 24;

}  // namespace

int layer_rects_tables(const RectsIn &in, RectsTables &out)
{
    out = RectsTables{};
    if (in.flags & ~(uint32_t)FR_LAYER_SRGB) return set_error(FR_E_INVALID, "unknown flag bits 0x%x", in.flags & ~(uint32_t)FR_LAYER_SRGB);
    if (const int rc = layer_image_check("dst", in.dst, in.dst_stride)) return rc;
    if (in.dst_rows > LAYER_MAX_ROWS) return set_error(FR_E_UNSUPPORTED, "an image of more than 2^31 - 1 rows");
    if (in.n_rects && !in.rects) return set_error(FR_E_INVALID, "rects is NULL");
    out.dst_vec = !(in.dst & 15u) && !(in.dst_stride % LAYER_LANE_PX);

    // clip to the image, in 1/64 pixel (stride <= 2^26, rows < 2^31: no overflow in int64)
    const int64_t w64 = std::min<int64_t>(64 * (int64_t)in.dst_stride, RECTS_MAX_EDGE), h64 = std::min<int64_t>(64 * (int64_t)in.dst_rows, RECTS_MAX_EDGE);
    uint64_t pairs = 0, most = 0;                          // all (tile, rectangle) pairs; the tiles of the largest rectangle
    for (uint32_t j = 0; j < in.n_rects; ++j) {
        const fr_layer_rect &r = in.rects[j];
        const int64_t x0 = std::clamp<int64_t>(r.x0, 0, w64), x1 = std::clamp<int64_t>(r.x1, 0, w64);
        const int64_t y0 = std::clamp<int64_t>(r.y0, 0, h64), y1 = std::clamp<int64_t>(r.y1, 0, h64);
        if (x0 >= x1 || y0 >= y1 || r.rgba[3] == 0) continue;  // empty, inverted, clipped away or transparent: valid, draws nothing
        const uint64_t n = (uint64_t)(((x1 - 1) >> TILE_X_SHIFT) - (x0 >> TILE_X_SHIFT) + 1) * (uint64_t)(((y1 - 1) >> TILE_Y_SHIFT) - (y0 >> TILE_Y_SHIFT) + 1);
        pairs += n;                                        // (n < 2^38, n_rects < 2^32: no overflow)
        most = std::max(most, n);
        if (pairs <= RECTS_MAX_PAIRS)                      // beyond, the call is refused below: keep no more records
            out.recs.push_back(RectRec{(uint32_t)x0, (uint32_t)y0, (uint32_t)x1, (uint32_t)y1,
                                       (uint32_t)r.rgba[0] | (uint32_t)r.rgba[1] << 8 | (uint32_t)r.rgba[2] << 16 | (uint32_t)r.rgba[3] << 24, j, {0, 0}});
    }
    if (most > LAYER_MAX_TILES) return set_error(FR_E_UNSUPPORTED, "the rectangles meet more than 2^22 tiles; split the call");
    if (pairs > RECTS_MAX_PAIRS) return set_error(FR_E_UNSUPPORTED, "more than 2^24 (tile, rectangle) pairs; split the call");

    if (out.recs.empty()) return FR_OK;

    // the tiles that hold them all: columns [tx0, tx0 + nx), rows [ty0, ty0 + ny)
    uint32_t tx0 = UINT32_MAX, ty0 = UINT32_MAX, tx1 = 0, ty1 = 0;
    for (const RectRec &c : out.recs) {
        tx0 = std::min(tx0, c.x0 >> TILE_X_SHIFT), tx1 = std::max(tx1, (c.x1 - 1) >> TILE_X_SHIFT);
        ty0 = std::min(ty0, c.y0 >> TILE_Y_SHIFT), ty1 = std::max(ty1, (c.y1 - 1) >> TILE_Y_SHIFT);
    }
    const uint64_t nx = tx1 - tx0 + 1, ny = ty1 - ty0 + 1;
    auto each_pair = [&](auto &&f) {                       // f(tile row, tile column, record), record by record
        for (size_t k = 0; k < out.recs.size(); ++k) {
            const RectRec &c = out.recs[k];
            for (uint64_t ty = c.y0 >> TILE_Y_SHIFT; ty <= (c.y1 - 1) >> TILE_Y_SHIFT; ++ty)
                for (uint64_t tx = c.x0 >> TILE_X_SHIFT; tx <= (c.x1 - 1) >> TILE_X_SHIFT; ++tx) f(ty, tx, (uint32_t)k);
        }
    };
    if (nx * ny <= std::max<uint64_t>(4 * pairs, (uint64_t)1 << 16)) {
        // rectangles that lie close together, the usual call: a counting sort over those tiles.  at[t]: the pairs of tile t,
        // then where its next list entry goes; walking the records in order leaves every tile's list ascending.
        std::vector<uint32_t> at((size_t)(nx * ny), 0);
        each_pair([&](uint64_t ty, uint64_t tx, uint32_t) { at[(size_t)((ty - ty0) * nx + (tx - tx0))]++; });
        size_t n_tiles = 0;
        for (const uint32_t n : at) n_tiles += n != 0;
        if (n_tiles > LAYER_MAX_TILES) return set_error(FR_E_UNSUPPORTED, "the rectangles meet more than 2^22 tiles; split the call");
        out.tiles.reserve(n_tiles);
        uint32_t first = 0;
        for (size_t t = 0; t < at.size(); ++t) {
            const uint32_t n = at[t];
            if (n) out.tiles.push_back(RectTile{(uint32_t)(tx0 + t % nx) * LAYER_TILE_W, (uint32_t)(ty0 + t / nx) * LAYER_TILE_H, first, n});
            at[t] = first;
            first += n;
        }
        out.list.resize((size_t)pairs);
        each_pair([&](uint64_t ty, uint64_t tx, uint32_t k) { out.list[at[(size_t)((ty - ty0) * nx + (tx - tx0))]++] = k; });
        return FR_OK;
    }
    // rectangles far apart in a large image: every pair as a word, sorted: tile by tile, a tile's records ascending
    std::vector<uint64_t> keys;
    keys.reserve((size_t)pairs);
    each_pair([&](uint64_t ty, uint64_t tx, uint32_t k) { keys.push_back(((ty << KEY_X_BITS | tx) << KEY_REC_BITS) | k); });
    std::sort(keys.begin(), keys.end());
    size_t n_tiles = 0;
    for (size_t i = 0; i < keys.size(); ++i) n_tiles += i == 0 || (keys[i] >> KEY_REC_BITS) != (keys[i - 1] >> KEY_REC_BITS);
    if (n_tiles > LAYER_MAX_TILES) return set_error(FR_E_UNSUPPORTED, "the rectangles meet more than 2^22 tiles; split the call");
    out.tiles.reserve(n_tiles);
    out.list.reserve(keys.size());
    for (size_t i = 0; i < keys.size(); ++i) {
        const uint64_t tile = keys[i] >> KEY_REC_BITS;
        if (i == 0 || tile != (keys[i - 1] >> KEY_REC_BITS))
            out.tiles.push_back(RectTile{(uint32_t)(tile & ((1u << KEY_X_BITS) - 1)) * LAYER_TILE_W, (uint32_t)(tile >> KEY_X_BITS) * LAYER_TILE_H, (uint32_t)i, 0});
        out.tiles.back().count++;
        out.list.push_back((uint32_t)(keys[i] & ((1u << KEY_REC_BITS) - 1)));
    }
    return FR_OK;
}

}  // namespace fr

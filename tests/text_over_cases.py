"""Exact cases for FR_TEXT_OVER text plans (include/fr_raster.h), built on the public helpers of tests/text_block_cases.py:
block glyphs whose edges lie on sample boundaries, so every pixel's lit samples are known from the geometry and the
expected bytes are computed in Python integers, with no rasteriser in between."""
import numpy as np

import text_block_cases as B
from font_renderer_amd import render_glyph as rg
from text_twin import alpha_over


def _apply(srgb, state, colour):
    """one sample state (..., 4) updated by an instance's colour (..., 4): R G B by the plan's blend, alpha source-over"""
    out = np.empty_like(state)
    out[..., :3] = (B.blend_srgb if srgb else B.blend_rgba)(colour[..., :3], state[..., :3], colour[..., 3:])
    out[..., 3] = alpha_over(state[..., 3], colour[..., 3])
    return out


def _colours(k1, k2):
    """the two translucent colours of the pair (k1, k2): every channel and both alphas vary with both counts"""
    one = np.stack([(13 * k1 + 7 * k2 + 40) % 256, (13 * k1 + 7 * k2 + 90) % 256, (13 * k1 + 7 * k2 + 140) % 256,
                    (37 * k1 + 91 * k2 + 60) % 256], axis=-1)
    two = np.stack([(29 * k1 + 91 * k2 + 3) % 256, (29 * k1 + 91 * k2 + 53) % 256, (29 * k1 + 91 * k2 + 103) % 256,
                    (101 * k1 + 53 * k2 + 129) % 256], axis=-1)
    return one, two


CLEARS = np.array([(0, 0, 0, 0), (0, 0, 0, 0), (200, 17, 99, 64), (200, 17, 99, 64)], np.uint8)


def partial_cover_case(n, ex, srgb):
    """Two translucent placements on the same 8 pixels for every (k1, k2) in 0 .. n^2: cover(k1, 8, n) in colour one and
    cover(k2, 8, n) in colour two (k = 0: no placement), at row k1, columns 8 k2 .. 8 k2 + 7 of a run.  The samples of
    cover(k) are the first k of the pixel in row order from the bottom, so the two sets are nested: min(k1, k2) samples
    take both colours in placement order, |k1 - k2| take one, the rest keep the clear colour.  Four runs: the pair in the
    order (one, two) and (two, one), over the clear colours (0, 0, 0, 0) and (200, 17, 99, 64).  Centre phase, scale 1/8.
    The pixels with k1 = 0 or k2 = 0 over the transparent clear hold consequence 5 of the header, asserted here."""
    nn = n * n
    glyphs = [B.cover(k, 8, n) for k in range(1, nn + 1)]
    h, w = nn + 1, 8 * (nn + 1)
    K1 = np.broadcast_to(np.arange(h, dtype=np.int64)[:, None], (h, w))
    K2 = np.broadcast_to((np.arange(w, dtype=np.int64) // 8)[None, :], (h, w))
    one, two = _colours(K1, K2)
    rows, rgba, runs = [], [], []
    want = np.full((1 + 4 * (h + 1), w + 2, 4), B.SENT, np.int64)
    for r in range(4):
        swapped = bool(r & 1)
        first = len(rows)
        for k1 in range(nn + 1):
            for k2 in range(nn + 1):
                c1, c2 = _colours(np.int64(k1), np.int64(k2))
                pair = [(k1, c1), (k2, c2)]
                for k, c in (pair[::-1] if swapped else pair):
                    if k:
                        rows.append((k - 1, 64 * 8 * k2, k1 + 1))
                        rgba.append(tuple(int(v) for v in c))
        oy = 1 + r * (h + 1)
        runs.append((first, len(rows) - first, w, h, 1, oy, 0.125))
        start = np.broadcast_to(CLEARS[r].astype(np.int64), (h, w, 4))
        (ka, ca), (kb, cb) = ((K2, two), (K1, one)) if swapped else ((K1, one), (K2, two))       # a is placed first
        both, only_a, only_b = np.minimum(ka, kb), np.maximum(ka - kb, 0), np.maximum(kb - ka, 0)
        rest = nn - np.maximum(ka, kb)
        parts = [(both[..., None], _apply(srgb, _apply(srgb, start, ca), cb)), (only_a[..., None], _apply(srgb, start, ca)),
                 (only_b[..., None], _apply(srgb, start, cb)), (rest[..., None], start)]
        img = np.empty((h, w, 4), np.int64)
        img[..., :3] = (B.mix_srgb if srgb else B.mix_rgba)([(k, v[..., :3]) for k, v in parts], n)
        img[..., 3] = B.mix_rgba([(k[..., 0], v[..., 3]) for k, v in parts], n)
        if not CLEARS[r].any():                               # consequence 5: one instance over (0, 0, 0, 0)
            assert np.array_equal(img[0, :, 3], (K2[0] * two[0, :, 3] + nn // 2) // nn)
            assert np.array_equal(img[:, 0, 3], (K1[:, 0] * one[:, 0, 3] + nn // 2) // nn)
        want[oy:oy + h, 1:1 + w] = img
    assert len({int(v) for v in np.unique(want[..., 3])}) > 32
    places = rg.make_places_ex([(g, x, 64 * y, 0.0, 0.0) for g, x, y in rows]) if ex else rg.make_places(rows)
    return B.ColourCase(glyphs=glyphs, places=places, rgba=np.array(rgba, np.uint8), runs=rg.make_runs(runs), clears=CLEARS,
                        start=np.full(want.shape, B.SENT, np.uint8), want=want.astype(np.uint8), n=n, one=one, two=two)


def every_alpha_pair_case(srgb, seed=3):
    """Every (a, A) on the device: n = 1, FR_TEXT_LOAD, a 256 x 256 image whose row r holds alpha r and noise R G B;
    placement k is a one-pixel-wide, 256-pixel-high block on column k with colour (noise, A = k).  Even font units, scale
    1/8, so the block's edges lie on pixel boundaries and the centre-phase samples inside them.  `want_alpha` is the
    definition in integers; R G B must equal the plan without the flag (the caller renders it)."""
    rng = np.random.default_rng(seed)
    glyphs = [B.BlockGlyph("column", [B.rect(0, 0, 8, 8 * 256)])]
    rows = [(0, 64 * k, 256) for k in range(256)]
    rgba = rng.integers(0, 256, (256, 4)).astype(np.uint8)
    rgba[:, 3] = np.arange(256)
    start = rng.integers(0, 256, (256, 256, 4)).astype(np.uint8)
    start[..., 3] = np.arange(256, dtype=np.uint8)[:, None]
    r, k = np.meshgrid(np.arange(256, dtype=np.int64), np.arange(256, dtype=np.int64), indexing="ij")
    want_alpha = (255 * k + r * (255 - k) + 127) // 255
    c0, r0, cw, ch = B.place_cell(glyphs[0].box, B.Fr(1, 8), B.Fr(0), 64 * 5, 64 * 256)
    assert (c0, r0) == (5, 0) and cw >= 1 and ch >= 256
    return B.ColourCase(glyphs=glyphs, places=rg.make_places(rows), rgba=rgba, runs=rg.make_runs([(0, 256, 256, 256, 0, 0, 0.125)]),
                        clears=None, start=start, want_alpha=want_alpha.astype(np.uint8), srgb=srgb)

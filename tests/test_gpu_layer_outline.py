"""fr_layer_outline on the GPU (include/fr_raster.h).  The expected image never comes from the code under test: it is the
numpy twin of the definition (tests/layer_outline_ref.py, itself held to a brute-force loop, to exact weights and to the
header's consequences by tests/test_layer_outline_ref.py), or fr_layer_shadow where the header promises its bytes.
Destinations are sentinel-filled with guard rows around them, and whole arrays are compared, so a byte written outside the
rectangle fails, and so does an unwritten pixel inside it; the layer is compared with its copy afterwards."""
import numpy as np
import pytest

import font_renderer_amd as fr
import layer_outline_ref as orf
import layer_ref as lr
import layer_shadow_ref as sr
import text_gpu as tg
from fixtures import load_font
from font_renderer_amd import _lib as L
from layer_gpu import SENT, Guarded

pytestmark = pytest.mark.gpu

KINDS = (orf.GROW, orf.RING, orf.INNER, orf.SHRINK)
RADII = [1, 8, 15, 16, 17, 40, 100, 256]
_planes = {}


def planes(layer, window, rho):
    """the twin's four alpha planes of a window, computed once per (layer, window, radius)"""
    key = (id(layer), window, rho)
    if key not in _planes:
        sx, sy, w, h = window
        _planes[key] = (layer, orf.alpha_planes(layer[sy:sy + h, sx:sx + w, 3], rho))      # (the layer is kept: its id stays its own)
    return _planes[key][1]


def _dev(layer, dst_shape, src_skip=0, dst_skip=0):
    return Guarded(np.full(dst_shape + (4,), SENT, np.uint8), layer, dst_skip, src_skip)


def _outline(ctx, d, window, rect, offset, rho, kind, rgba, srgb=False, flags=0):
    fr.layer_outline(ctx, d.src, d.layer.shape[1], d.layer.shape[0], d.dst, d.image.shape[1], d.image.shape[0], window, rect, offset, rho, kind, rgba, srgb,
                     flags)


def _run(ctx, layer, dst_shape, window, rect, offset, rho, kind, rgba, srgb=False, src_skip=0, dst_skip=0):
    """one call on fresh buffers -> (got, want)"""
    d = _dev(layer, dst_shape, src_skip, dst_skip)
    _outline(ctx, d, window, rect, offset, rho, kind, rgba, srgb)
    p = planes(layer, tuple(window), rho) if window[2] and window[3] else None
    return d.result(ctx), orf.outline(layer, d.image, window, rect, offset, rho, kind, rgba, srgb, p)


def sparse(rng, shape):
    """a text-like premultiplied layer: 60 % (0, 0, 0, 0), partial alphas, and some blocks of 255"""
    a = rng.integers(1, 256, shape)
    a[rng.random(shape) < 0.6] = 0
    for _ in range(6):
        y, x = rng.integers(0, shape[0] - 8), rng.integers(0, shape[1] - 12)
        a[y:y + rng.integers(3, 9), x:x + rng.integers(3, 13)] = 255
    c = rng.integers(0, 256, shape + (3,)) * a[..., None] // 255
    return np.concatenate([c, a[..., None]], -1).astype(np.uint8)


@pytest.fixture(scope="module")
def layers():
    rng = np.random.default_rng(29)
    return {"small": sparse(rng, (41, 97)), "wide": sparse(rng, (80, 300))}


# ---- impulses ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("first", range(0, 257, 43))
def test_an_impulse_gives_the_weights(ctx, first):
    """one pixel of alpha 255, GROW, white: the alpha plane of a (2 R + 5)^2 rectangle is the table K, for every radius"""
    one = np.zeros((1, 1, 4), np.uint8)
    one[0, 0, 3] = 255
    for rho in range(first, min(first + 43, 257)):
        R = orf.reach(rho)
        n = 2 * R + 5
        d = _dev(one, (n, n))
        _outline(ctx, d, (0, 0, 1, 1), (0, 0, n, n), (R + 2, R + 2), rho, orf.GROW, (255, 255, 255, 255))
        want = np.zeros((n, n), np.uint8)
        want[2:2 + 2 * R + 1, 2:2 + 2 * R + 1] = orf.weights(rho)
        got = d.result(ctx)
        assert np.array_equal(got, np.repeat(want[..., None], 4, -1)), (rho, np.argwhere(got[..., 3] != want)[:4])


# ---- tile borders, kinds and the two store paths ----------------------------------------------------------------------------
@pytest.mark.parametrize("rho", RADII)
def test_sparse_layer_across_tile_borders(ctx, layers, rho):
    """a 150 x 70 window of a wider layer into a rectangle padded by the reach (three tiles by two): every kind, 16-byte
    stores (rows of 192, the rectangle on and off the grid) and single pixels (rows of 191), both colour spaces"""
    R = orf.reach(rho)
    window = (101, 7, 150, 70)
    for kind in KINDS:
        for stride, dst_x, dst_skip, srgb in ((192, 0, 0, False), (192, 1, 0, True), (192, 2, 3, False), (191, 3, 1, True)):
            rect = (dst_x, 2, 150 + 2 * R, 70 + 2 * R)
            cols = stride + (4 if rect[0] + rect[2] > stride else 0)
            got, want = _run(ctx, layers["wide"], (rect[1] + rect[3] + 1, cols), window, rect, (R, R), rho, kind, (30, 144, 255, 200), srgb, dst_skip=dst_skip)
            assert np.array_equal(got, want), (rho, kind, stride, dst_x, np.argwhere(got != want)[:4])


@pytest.mark.parametrize("dst_w", range(1, 10))
def test_rectangle_widths(ctx, layers, dst_w):
    for rho, kind in ((17, orf.GROW), (100, orf.RING), (40, orf.INNER), (8, orf.SHRINK)):
        for dst_x, stride in ((0, 132), (3, 132), (6, 131)):
            got, want = _run(ctx, layers["small"], (50, stride), (0, 0, 97, 41), (dst_x, 2, dst_w, 45), (-17, 3), rho, kind, (255, 0, 128, 255), True)
            assert np.array_equal(got, want), (rho, kind, dst_x, stride, np.argwhere(got != want)[:4])


# (layer, window, rect as a function of the reach, offset as a function of the reach)
GEOMETRY = {
    "larger_than_the_reach": ("small", (0, 0, 97, 41), lambda R: (1, 2, 97 + 2 * R + 9, 41 + 2 * R + 7), lambda R: (R + 4, R + 3)),
    "unpadded": ("small", (0, 0, 97, 41), lambda R: (5, 3, 97, 41), lambda R: (0, 0)),
    "cut_left_top": ("small", (0, 0, 97, 41), lambda R: (0, 0, 60, 30), lambda R: (-20, -15)),
    "cut_right_bottom": ("small", (0, 0, 97, 41), lambda R: (4, 4, 80, 35), lambda R: (40, 20)),
    "far_away": ("small", (0, 0, 97, 41), lambda R: (3, 3, 50, 20), lambda R: (-(97 + R), 0)),
    "far_away_up": ("small", (0, 0, 97, 41), lambda R: (3, 3, 50, 20), lambda R: (0, 20 + R)),
    "just_in_reach": ("small", (0, 0, 97, 41), lambda R: (3, 3, 50, 20), lambda R: (-(97 + R - 1), -(41 + R - 1))),
    "window_in_a_wider_layer": ("wide", (101, 13, 120, 40), lambda R: (0, 0, 120 + 2 * R, 40 + 2 * R), lambda R: (R, R)),
    "window_at_the_layers_corner": ("wide", (203, 39, 97, 41), lambda R: (2, 2, 100, 60), lambda R: (1, 5)),
    "window_at_the_layers_origin": ("wide", (0, 0, 97, 41), lambda R: (2, 2, 120, 60), lambda R: (R, 5)),
    "the_whole_layer": ("wide", (0, 0, 300, 80), lambda R: (0, 0, 300 + 2 * R, 80 + 2 * R), lambda R: (R, R)),
}


@pytest.mark.parametrize("rho", [0, 17, 100, 256])
@pytest.mark.parametrize("case", sorted(GEOMETRY))
def test_geometry(ctx, layers, case, rho):
    """windows that touch the layer's edges (outside counts as 0: for INNER and SHRINK the window's edge erodes), rectangles
    larger than the reach, clipped inside it and wholly out of it, which gives zeros"""
    name, window, rect, offset = GEOMETRY[case]
    R = orf.reach(rho)
    rect, offset = rect(R), offset(R)
    cols = (rect[0] + rect[2] + 1 + 3) // 4 * 4
    for kind in KINDS:
        got, want = _run(ctx, layers[name], (rect[1] + rect[3] + 2, cols), window, rect, offset, rho, kind, (30, 144, 255, 200), kind % 2 == 1)
        assert np.array_equal(got, want), (case, rho, kind, np.argwhere(got != want)[:4])
        inside = want[rect[1]:rect[1] + rect[3], rect[0]:rect[0] + rect[2]]
        if case in ("far_away", "far_away_up"):
            assert not inside.any()
        if case == "just_in_reach" and kind in (orf.INNER, orf.SHRINK) and rho:
            assert not inside.any()                                 # R >= 1: the rectangle lies beyond the window
        if case == "just_in_reach":
            assert (inside[..., 3] != 0).sum() <= 1
        if case == "the_whole_layer" and kind == orf.SHRINK and rho >= 16:
            assert not inside[R:R + 1].any() and not inside[:, R:R + 1].any()       # the window's border erodes


def test_zero_sizes(ctx, layers):
    """dst_w or dst_h of 0 writes nothing; a window without area writes zeros over the rectangle, for every kind"""
    d = _dev(layers["small"], (50, 132))
    _outline(ctx, d, (0, 0, 97, 41), (7, 7, 0, 30), (0, 0), 40, orf.GROW, (1, 2, 3, 255))
    _outline(ctx, d, (0, 0, 97, 41), (1000, 1000, 30, 0), (0, 0), 40, orf.RING, (1, 2, 3, 255))
    assert np.array_equal(d.result(ctx), d.image)
    want = d.image.copy()
    for kind in KINDS:
        _outline(ctx, d, (500, 500, 0, 41) if kind % 2 else (0, 0, 97, 0), (7 + 30 * kind, 8, 29, 30), (0, 0), 40, kind, (1, 2, 3, 255))
        want[8:38, 7 + 30 * kind:36 + 30 * kind] = 0
    assert np.array_equal(d.result(ctx), want)


def test_translation(ctx, layers):
    layer = layers["small"]
    for rho, kind in ((40, orf.GROW), (24, orf.INNER)):
        base, want = _run(ctx, layer, (80, 132), (0, 0, 97, 41), (0, 0, 132, 80), (12, 12), rho, kind, (200, 100, 50, 220))
        assert np.array_equal(base, want)
        for dx, dy in ((1, 0), (0, 1), (3, 2), (-1, -4)):
            moved, _ = _run(ctx, layer, (80, 132), (0, 0, 97, 41), (0, 0, 132, 80), (12 + dx, 12 + dy), rho, kind, (200, 100, 50, 220))
            assert np.array_equal(moved, np.roll(base, (dy, dx), (0, 1))), (kind, dx, dy)  # padded by more than the reach plus the move


# ---- symmetry ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rho,kind", [(17, orf.GROW), (100, orf.RING), (56, orf.INNER), (33, orf.SHRINK)])
def test_the_eight_symmetries(ctx, layers, rho, kind):
    """a transposed or mirrored window gives the transposed or mirrored image"""
    part = layers["small"][2:39, 3:93]
    base = None
    for flip_x in (False, True):
        for flip_y in (False, True):
            for swap in (False, True):
                a = part[:, ::-1] if flip_x else part
                a = a[::-1] if flip_y else a
                a = np.ascontiguousarray(a.transpose(1, 0, 2) if swap else a)
                h, w = a.shape[:2]
                got, _ = _run(ctx, a, (h + 40, w + 40 + (-w) % 4), (0, 0, w, h), (0, 0, w + 40, h + 40), (20, 20), rho, kind, (10, 200, 30, 180))
                got = got[:, :w + 40]
                got = got.transpose(1, 0, 2) if swap else got
                got = got[::-1] if flip_y else got
                got = got[:, ::-1] if flip_x else got
                if base is None:
                    base = got
                    want = orf.outline_rect(a, (0, 0, w, h), (w + 40, h + 40), (20, 20), rho, kind, (10, 200, 30, 180))
                    assert np.array_equal(got, want)
                assert np.array_equal(got, base), (flip_x, flip_y, swap)


# ---- against fr_layer_shadow -----------------------------------------------------------------------------------------------
def _shadow_bytes(ctx, layer, dst_shape, window, rect, offset, spread, rgba, srgb):
    d = _dev(layer, dst_shape)
    fr.layer_shadow(ctx, d.src, layer.shape[1], layer.shape[0], d.dst, dst_shape[1], dst_shape[0], window, rect, offset, spread, 0, 0, rgba, srgb)
    return d.result(ctx)


@pytest.mark.parametrize("srgb", [False, True], ids=["unorm", "srgb"])
def test_radius_0_is_the_shadow_without_a_stage(ctx, layers, srgb):
    """consequence 1: GROW and SHRINK at radius 0 are fr_layer_shadow's bytes, RING and INNER zeros"""
    layer, window, rect, colour = layers["wide"], (11, 3, 200, 70), (3, 2, 210, 76), (30, 144, 255, 200)
    shadow = _shadow_bytes(ctx, layer, (80, 216), window, rect, (4, 3), 0, colour, srgb)
    for kind in KINDS:
        d = _dev(layer, (80, 216))
        _outline(ctx, d, window, rect, (4, 3), 0, kind, colour, srgb)
        want = shadow
        if kind in (orf.RING, orf.INNER):
            want = d.image.copy()
            want[2:78, 3:213] = 0
        assert np.array_equal(d.result(ctx), want), kind


@pytest.mark.parametrize("rho", [1, 16, 17, 40, 100, 128])
def test_the_sandwich(ctx, layers, rho):
    """consequence 4: shadow(no stage) <= GROW <= shadow(spread = R, no blur) pointwise in alpha, all three from the device"""
    R = orf.reach(rho)
    layer, window, colour = layers["small"], (0, 0, 97, 41), (255, 255, 255, 255)
    shape, rect = (41 + 2 * R + 4, 132), (1, 2, 97 + 2 * R + 2, 41 + 2 * R + 2)
    low = _shadow_bytes(ctx, layer, shape, window, rect, (R + 1, R + 1), 0, colour, False)[..., 3]
    high = _shadow_bytes(ctx, layer, shape, window, rect, (R + 1, R + 1), R, colour, False)[..., 3]
    d = _dev(layer, shape)
    _outline(ctx, d, window, rect, (R + 1, R + 1), rho, orf.GROW, colour)
    grow = d.result(ctx)[..., 3]
    assert (low <= grow).all() and (grow <= high).all()
    assert (grow < high).any()                                      # the disc is smaller than the square


# ---- the tint over its domain ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("srgb", [False, True], ids=["unorm", "srgb"])
def test_tint_over_its_domain(ctx, srgb):
    """a 256 x 4 window whose alpha is the column, radius 0, GROW: 256 calls with A = 0 .. 255 cover every (alpha, A), 86 calls
    at A = 255 whose colour bytes sweep 0 .. 255 cover every (C, a); each call has its own four rows of one destination"""
    layer = np.zeros((4, 256, 4), np.uint8)
    layer[..., 3] = np.arange(256)[None, :]
    layer[..., :3] = 77
    colours = [((3 * A) % 256, (255 - A) % 256, (A * 7 + 1) % 256, A) for A in range(256)]
    colours += [(k, (k + 86) % 256, (k + 172) % 256, 255) for k in range(86)]
    d = _dev(layer, (4 * len(colours), 256))
    want = d.image.copy()
    for i, c in enumerate(colours):
        _outline(ctx, d, (0, 0, 256, 4), (0, 4 * i, 256, 4), (0, 0), 0, orf.GROW, c, srgb)
        want[4 * i:4 * i + 4] = sr.tint(layer[..., 3].astype(np.int64), c, srgb)
    got = d.result(ctx)
    assert np.array_equal(got, want), np.argwhere(got != want)[:4]


# ---- end to end ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def text_line(ctx):
    """one real-font line rendered with FR_TEXT_OVER over (0, 0, 0, 0), in both colour spaces: {srgb: (layer, w, h)}"""
    from font_renderer_amd.text import _line
    font = load_font("DejaVuSans.ttf", allow_hinted=True)
    gs, places, runs, w, h = _line(font, "Outline fjord, quay!", 19)
    cols = tg.colours(len(places), 5, opaque=True)
    out = {}
    dgs = fr.DeviceGlyphSet(ctx, gs)
    try:
        for srgb in (False, True):
            flags = fr.FR_TEXT_OVER | (fr.FR_TEXT_SRGB if srgb else 0)
            layer = tg.render_rgba(ctx, dgs, places, cols, runs, [(0, 0, 0, 0)], np.zeros((h, w, 4), np.uint8), 1, True, flags)
            assert layer[..., 3].max() == 255 and (layer[..., 3] == 0).any()
            out[srgb] = (layer, w, h)
    finally:
        dgs.close()
    return out


@pytest.mark.parametrize("srgb", [False, True], ids=["unorm", "srgb"])
def test_outlined_text_over_a_frame(ctx, text_line, srgb):
    """the line's outline (rho = 24, GROW, a translucent colour) composited onto a noise frame with fr_layer_over, then the
    text over it, in one stream with no sync between the calls == layer_ref.composite of the twin's outline and the same
    layer, byte for byte"""
    import torch
    layer, w, h = text_line[srgb]
    R, tx, ty = 2, 9, 7
    H, W = h + 2 * R + 10, (w + 2 * R + 12 + 3) // 4 * 4
    frame = tg.noise((H, W), 9)
    colour = (250, 240, 20, 230)
    dev_layer = torch.from_numpy(layer).to("cuda:0")
    dev_outline = torch.full((H, W, 4), SENT, dtype=torch.uint8, device="cuda:0")
    dev_frame = torch.from_numpy(frame.copy()).to("cuda:0")
    torch.cuda.synchronize()
    fr.layer_outline(ctx, dev_layer.data_ptr(), w, h, dev_outline.data_ptr(), W, H, (0, 0, w, h), (0, 0, W, H), (tx, ty), 24, orf.GROW, colour, srgb)
    fr.layer_over(ctx, dev_outline.data_ptr(), W, H, dev_frame.data_ptr(), W, H, fr.make_blits([(0, 0, W, H, 0, 0, 255)]), srgb)
    fr.layer_over(ctx, dev_layer.data_ptr(), w, h, dev_frame.data_ptr(), W, H, fr.make_blits([(0, 0, w, h, tx, ty, 255)]), srgb)
    ctx.sync()
    outline = orf.outline_rect(layer, (0, 0, w, h), (W, H), (tx, ty), 24, orf.GROW, colour, srgb)
    assert np.array_equal(dev_outline.cpu().numpy(), outline)
    want = lr.composite(layer, lr.composite(outline, frame, [(0, 0, W, H, 0, 0, 255)], srgb), [(0, 0, w, h, tx, ty, 255)], srgb)
    got = dev_frame.cpu().numpy()
    assert np.array_equal(got, want), np.argwhere(got != want)[:4]
    assert not np.array_equal(got, frame) and outline[..., 3].max() == 230


@pytest.mark.parametrize("kind,rho", [(orf.RING, 20), (orf.INNER, 12)], ids=["hollow", "inner_line"])
def test_hollow_text_and_an_inner_line(ctx, text_line, kind, rho):
    """RING alone over a frame is hollow text; INNER goes over the text itself"""
    import torch
    layer, w, h = text_line[False]
    R = orf.reach(rho)
    H, W = h + 2 * R, (w + 2 * R + 3) // 4 * 4
    frame = tg.noise((H, W), 11)
    dev_layer = torch.from_numpy(layer).to("cuda:0")
    dev_line = torch.full((H, W, 4), SENT, dtype=torch.uint8, device="cuda:0")
    dev_frame = torch.from_numpy(frame.copy()).to("cuda:0")
    torch.cuda.synchronize()
    blits = [(0, 0, W, H, 0, 0, 255)]
    fr.layer_outline(ctx, dev_layer.data_ptr(), w, h, dev_line.data_ptr(), W, H, (0, 0, w, h), (0, 0, W, H), (R, R), rho, kind, (255, 255, 255, 255))
    if kind == orf.INNER:
        fr.layer_over(ctx, dev_layer.data_ptr(), w, h, dev_frame.data_ptr(), W, H, fr.make_blits([(0, 0, w, h, R, R, 255)]))
    fr.layer_over(ctx, dev_line.data_ptr(), W, H, dev_frame.data_ptr(), W, H, fr.make_blits(blits))
    ctx.sync()
    line = orf.outline_rect(layer, (0, 0, w, h), (W, H), (R, R), rho, kind, (255, 255, 255, 255))
    assert np.array_equal(dev_line.cpu().numpy(), line) and line[..., 3].max() > 128
    want = frame
    if kind == orf.INNER:
        want = lr.composite(layer, want, [(0, 0, w, h, R, R, 255)])
    want = lr.composite(line, want, blits)
    assert np.array_equal(dev_frame.cpu().numpy(), want)
    if kind == orf.RING:                                            # hollow: where the text is opaque the ring is empty
        assert not line[R:R + h, R:R + w, 3][layer[..., 3] == 255].any()


def test_rgba_outline_method(ctx, layers):
    layer = fr.RGBA(97, 41, layers["small"].reshape(-1, 4).copy())
    out = layer.outline(40, rgba=(0, 0, 0, 128), ctx=ctx)
    assert (out.width, out.height) == (103, 47)
    assert np.array_equal(out.as_3d(), orf.outline_rect(layers["small"], (0, 0, 97, 41), (103, 47), (3, 3), 40, orf.GROW, (0, 0, 0, 128)))
    out = layer.outline(17, kind=fr.FR_OUTLINE_INNER, rgba=(9, 8, 7, 255), offset=(2, 3), pad=8, srgb=True, ctx=ctx)
    assert (out.width, out.height) == (113, 57)
    assert np.array_equal(out.as_3d(), orf.outline_rect(layers["small"], (0, 0, 97, 41), (113, 57), (10, 11), 17, orf.INNER, (9, 8, 7, 255), True))


# ---- validation through the ABI --------------------------------------------------------------------------------------------
def test_refusals_leave_the_destination_untouched(ctx, layers):
    d = _dev(layers["small"], (50, 132))
    S, D = d.src, d.dst
    win, rect = (0, 0, 97, 41), (0, 0, 100, 50)

    def call(s=S, ss=97, srows=41, dp=D, ds=132, dr=50, window=win, rc=rect, rho=40, kind=orf.GROW, flags=0):
        fr.layer_outline(ctx, s, ss, srows, dp, ds, dr, window, rc, (0, 0), rho, kind, (1, 2, 3, 255), False, flags)

    cases = {
        "src NULL": (-1, "src", dict(s=0)),
        "dst NULL": (-1, "dst", dict(dp=0)),
        "outline NULL": (-1, "outline", dict(window=None)),
        "src not 4-byte aligned": (-1, "src", dict(s=S + 2, srows=40)),
        "dst not 4-byte aligned": (-1, "dst", dict(dp=D + 1, dr=49)),
        "src pitch beyond 2^26": (-1, "src", dict(ss=(1 << 26) + 1, srows=0)),
        "2^31 rows": (-4, "rows", dict(ds=0, dr=1 << 31, rc=(0, 0, 0, 0))),
        "window one pixel out": (-1, "window", dict(window=(1, 0, 97, 41))),
        "window one row out": (-1, "window", dict(window=(0, 1, 97, 41))),
        "rectangle one pixel out": (-1, "rectangle", dict(rc=(33, 0, 100, 50))),
        "rectangle one row out": (-1, "rectangle", dict(rc=(0, 1, 100, 50))),
        "radius 257": (-1, "radius", dict(rho=257)),
        "kind 4": (-1, "kind", dict(kind=4)),
        "unknown flag": (-1, "flag", dict(flags=2)),
        "a text flag": (-1, "flag", dict(flags=fr.FR_TEXT_OVER)),
        "the images alias": (-1, "overlap", dict(s=D, ss=132, srows=50)),
    }
    for what, (code, word, kw) in cases.items():
        with pytest.raises(fr.FrError) as e:
            call(**kw)
        assert e.value.code == code and word in str(e.value), (what, str(e.value))
    with pytest.raises(fr.FrError) as e:                               # NULL ctx
        L.check(L.load_library().fr_layer_outline(None, S, 97, 41, D, 132, 50, None, 0))
    assert e.value.code == -1 and "ctx" in str(e.value)
    assert np.array_equal(d.result(ctx), d.image)
    call(rho=256, kind=orf.SHRINK)                                     # the limits are valid
    assert np.array_equal(d.result(ctx), orf.outline(layers["small"], d.image, win, rect, (0, 0), 256, orf.SHRINK, (1, 2, 3, 255)))

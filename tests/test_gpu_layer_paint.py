"""fr_layer_paint on the GPU (include/fr_raster.h).  The expected image never comes from the code under test: it is the
numpy / Python-int twin of the definition (tests/layer_paint_ref.py, itself held to exact fractions and to the header's
consequences by tests/test_layer_paint_ref.py), or a route through fr_layer_rects, fr_layer_shadow and fr_layer_over.
Destinations sit between guard rows, the layer is compared with its copy after every call, and whole arrays are compared, so
a byte written outside the clipped rectangle fails."""
import math

import numpy as np
import pytest

import font_renderer_amd as fr
import layer_paint_ref as pr
from fixtures import load_font
from font_renderer_amd import _lib as L
from layer_gpu import SENT, Guarded, premultiplied

pytestmark = pytest.mark.gpu

TWO = [(0, (255, 0, 0, 255)), (65536, (0, 0, 255, 255))]
HARD = [(0, (250, 10, 60, 255)), (20000, (10, 250, 60, 255)), (20000, (0, 0, 0, 255)), (50000, (255, 255, 255, 90)), (50000, (40, 80, 160, 255))]
CLEAR = [(3000, (255, 200, 0, 255)), (30000, (0, 90, 255, 0)), (36000, (0, 90, 255, 0)), (65000, (200, 0, 255, 180))]
# every table entry differs from the next: seven steep segments, all opaque
STEEP = [(9362 * i, c + (255,)) for i, c in enumerate([(255, 0, 0), (0, 255, 0), (0, 0, 255), (255, 255, 0), (0, 255, 255), (255, 0, 255), (0, 0, 0), (255, 255, 255)])]


def _params(grad):
    kind, spread, (x0, y0, x1, y1), stops = grad
    if kind == pr.LINEAR:
        return fr.make_gradient_linear(x0, y0, x1, y1, stops, spread)
    assert y1 == 0
    return fr.make_gradient_radial(x0, y0, x1, stops, spread)


def _call(ctx, d, image, layer, window, dst, grad, srgb=False):
    src = (None, 0, 0) if layer is None else (d.src, layer.shape[1], layer.shape[0])
    fr.layer_paint(ctx, *src, d.dst, image.shape[1], image.shape[0], _params(grad), window, dst, srgb)


def _paint(ctx, image, layer, window, dst, grad, srgb=False, skip=0):
    """fr_layer_paint over guarded device copies of `image` (rows, stride, 4) and `layer` (or None: full coverage) -> the
    image after.  skip: pixels both device arrays are moved by, to leave the 16-byte grid."""
    d = Guarded(image, layer, dst_skip=skip, src_skip=skip)
    _call(ctx, d, image, layer, window, dst, grad, srgb)
    return d.result(ctx)


def _check(ctx, image, layer, window, dst, grad, srgb=False, skip=0, changed=True):
    got = _paint(ctx, image, layer, window, dst, grad, srgb, skip)
    want = pr.paint(image, layer, window, dst, grad, srgb)
    assert np.array_equal(got, want), np.argwhere(got != want)[:4]
    if changed is not None:
        assert np.array_equal(got, image) != changed
    return got


@pytest.fixture(scope="module")
def noise():
    """(images 40 x 300 and 40 x 301, a layer 40 x 300): cov takes 0, 255 and values between"""
    rng = np.random.default_rng(41)
    return {300: premultiplied(rng, (40, 300)), 301: premultiplied(rng, (40, 301))}, premultiplied(rng, (40, 300))


@pytest.mark.parametrize("stride,skip", [(300, 0), (301, 1)], ids=["aligned", "off_grid"])
@pytest.mark.parametrize("src", [True, False], ids=["layer", "full"])
@pytest.mark.parametrize("kind", [pr.LINEAR, pr.RADIAL], ids=["linear", "radial"])
@pytest.mark.parametrize("srgb", [False, True], ids=["unorm", "srgb"])
def test_every_instance(ctx, noise, srgb, kind, src, stride, skip):
    """the eight kernel instances over a 300 x 40 image, two tiles across and three down with a ragged right and bottom
    edge, the rectangle with a margin: rows of 300 on the 16-byte grid (the 16-byte path, ragged at both ends) and rows of
    301 one pixel off it (pixel by pixel)"""
    images, layer = noise
    grad = (pr.LINEAR, pr.REFLECT, (37, -11, 6001, 1733), CLEAR) if kind == pr.LINEAR else (pr.RADIAL, pr.REPEAT, (64 * 140 + 7, 64 * 17 - 9, 64 * 40 + 5, 0), CLEAR)
    _check(ctx, images[stride], layer if src else None, (3, 2, 290, 35) if src else (0, 0, 290, 35), (5, 3), grad, srgb, skip)


LINEAR = {"horizontal": (100, 0, 64 * 280, 0), "vertical": (0, 64 * 2, 0, 64 * 37), "diagonal": (64, 64, 64 + 2048, 64 + 2048), "reversed": (64 * 290, 64 * 30, 64 * 10, 64 * 5),
          "shallow": (37, -11, 19001, 1733)}


@pytest.mark.parametrize("name", sorted(LINEAR))
def test_linear_gradients(ctx, noise, name):
    images, layer = noise
    got = _check(ctx, images[300], layer, (0, 0, 300, 40), (0, 0), (pr.LINEAR, pr.PAD, LINEAR[name], TWO), name == "shallow")
    if name == "horizontal":                                   # consequence 5 on full coverage: identical rows
        full = _check(ctx, images[300] * 0, None, (0, 0, 300, 40), (0, 0), (pr.LINEAR, pr.PAD, LINEAR[name], TWO))
        assert (full == full[0]).all() and not np.array_equal(got, full)


@pytest.mark.parametrize("r", [64, 6400])
@pytest.mark.parametrize("centre", [(64 * 150 + 32, 64 * 20 + 32), (64 * 150, 64 * 20), (-64 * 40 - 13, 64 * 70 + 5)], ids=["pixel_centre", "pixel_corner", "outside"])
def test_radial_gradients(ctx, noise, centre, r):
    images, layer = noise
    _check(ctx, images[300], layer, (0, 0, 300, 40), (0, 0), (pr.RADIAL, pr.REFLECT if r == 64 else pr.PAD, (*centre, r, 0), STEEP if r == 64 else TWO), r == 64)
    if centre[0] > 0:                                          # consequence 5 on full coverage: symmetric about the centre
        full = _check(ctx, images[300] * 0, None, (0, 0, 300, 40), (0, 0), (pr.RADIAL, pr.REPEAT, (*centre, r, 0), STEEP))
        lo = 1 if centre[0] % 64 else 0                        # a pixel centre at column 150: columns 1 .. 299; a corner: 0 .. 299
        assert np.array_equal(full[:, lo:], full[:, lo:][:, ::-1]) and np.array_equal(full[lo:], full[lo:][::-1])


@pytest.mark.parametrize("stops", [HARD, CLEAR], ids=["hard_edges", "transparent_stop"])
@pytest.mark.parametrize("spread", [pr.PAD, pr.REPEAT, pr.REFLECT], ids=["pad", "repeat", "reflect"])
@pytest.mark.parametrize("srgb", [False, True], ids=["unorm", "srgb"])
def test_spreads_and_stops(ctx, noise, srgb, spread, stops):
    """a short gradient in the middle of the image, so that t runs from well below 0 to well above 65536"""
    images, layer = noise
    _check(ctx, images[300], layer, (0, 0, 300, 40), (0, 0), (pr.LINEAR, spread, (64 * 130, 64 * 10, 64 * 170, 64 * 25), stops), srgb)
    _check(ctx, images[300], None, (0, 0, 300, 40), (0, 0), (pr.RADIAL, spread, (64 * 100 + 9, 64 * 20, 64 * 30, 0), stops), srgb)


@pytest.mark.parametrize("srgb", [False, True], ids=["unorm", "srgb"])
def test_empty_and_full_layers(ctx, noise, srgb):
    images, _ = noise
    grad = (pr.RADIAL, pr.REPEAT, (64 * 150, 64 * 20, 64 * 50, 0), STEEP)
    _check(ctx, images[300], np.zeros((40, 300, 4), np.uint8), (0, 0, 300, 40), (0, 0), grad, srgb, changed=False)
    # cov = 255 and A = 255: no bit of the destination reaches the result, whatever it holds
    solid = np.full((40, 300, 4), 255, np.uint8)
    a = _check(ctx, np.full((40, 300, 4), SENT, np.uint8), solid, (0, 0, 300, 40), (0, 0), grad, srgb)
    b = _check(ctx, np.full((40, 300, 4), 0xa4, np.uint8), solid, (0, 0, 300, 40), (0, 0), grad, srgb)
    assert np.array_equal(a, b) and (a[..., 3] == 255).all()
    # a transparent stop: A = 0 leaves the pixel as it is
    gone = _check(ctx, images[300], solid, (0, 0, 300, 40), (0, 0), (pr.LINEAR, pr.PAD, (0, 0, 64 * 300, 0), CLEAR), srgb)
    A = pr.table(CLEAR)[pr.parameter((pr.LINEAR, pr.PAD, (0, 0, 64 * 300, 0), CLEAR), 0, 0, 300, 1)[0] >> 6][:, 3]
    assert (A == 0).sum() > 10 and np.array_equal(gone[:, A == 0], images[300][:, A == 0])


CLIPS = {"negative_position": ((0, 0, 300, 40), (-7, -5)), "window_at_1_negative_position": ((1, 1, 299, 39), (-2, -1)), "over_the_right_and_bottom": ((0, 0, 300, 40), (200, 30)),
         "one_pixel_left": ((0, 0, 300, 40), (-299, -39)), "clipped_away_right": ((0, 0, 300, 40), (301, 0)), "clipped_away_above": ((0, 0, 300, 40), (0, -40)),
         "clipped_away_far": ((0, 0, 300, 40), (-2 ** 31, 2 ** 31 - 1)), "zero_width": ((0, 0, 0, 40), (5, 5))}


@pytest.mark.parametrize("stride,skip", [(300, 0), (301, 1)], ids=["aligned", "off_grid"])
@pytest.mark.parametrize("name", sorted(CLIPS))
def test_clipping(ctx, noise, name, stride, skip):
    images, layer = noise
    window, dst = CLIPS[name]
    for grad in ((pr.LINEAR, pr.REPEAT, (64, 64, 64 + 2048, 64 + 2048), HARD), (pr.RADIAL, pr.REFLECT, (64 * 290, 64 * 35, 64 * 9, 0), TWO)):
        changed = None if name == "one_pixel_left" else not (name.startswith("clipped") or name == "zero_width")     # (that pixel's cov may be 0)
        _check(ctx, images[stride], layer, window, dst, grad, True, skip, changed=changed)


def test_consequence_4_on_the_device(ctx, noise):
    images, layer = noise
    image = images[300]
    for grad, moved in [((pr.LINEAR, pr.REFLECT, (64, 64, 64 + 2048, 64 + 2048), HARD), (pr.LINEAR, pr.REFLECT, (128, 128, 128 + 2048, 128 + 2048), HARD)),
                        ((pr.RADIAL, pr.REPEAT, (1237, 911, 777, 0), STEEP), (pr.RADIAL, pr.REPEAT, (1301, 975, 777, 0), STEEP))]:
        a = _paint(ctx, image, layer, (0, 0, 290, 35), (2, 3), grad)
        b = _paint(ctx, np.roll(image, (1, 1), (0, 1)), layer, (0, 0, 290, 35), (3, 4), moved)
        assert np.array_equal(a[3:38, 2:292], b[4:39, 3:293]) and not np.array_equal(a, image)


@pytest.mark.parametrize("srgb", [False, True], ids=["unorm", "srgb"])
def test_consequence_1_on_the_device(ctx, noise, srgb):
    """one stop through full coverage == fr_layer_rects with the pixel-aligned rectangle of that colour, no twin involved"""
    images, _ = noise
    for stride, skip in ((300, 0), (301, 1)):
        image = images[stride]
        for colour in ((17, 250, 3, 255), (200, 90, 20, 141)):
            got = _paint(ctx, image, None, (0, 0, 280, 33), (9, 4), (pr.RADIAL, pr.REPEAT, (5, 5, 640, 0), [(40000, colour)]), srgb, skip)
            d = Guarded(image, dst_skip=skip)
            fr.layer_rects(ctx, d.dst, stride, 40, fr.make_rects([(64 * 9, 64 * 4, 64 * 289, 64 * 37, colour)]), srgb)
            assert np.array_equal(got, d.result(ctx)) and not np.array_equal(got, image)


def test_consequence_2_on_the_device(ctx, noise):
    """one stop and a layer, flags = 0 == fr_layer_shadow (no stage, that colour) of the window into a cleared layer,
    composited by fr_layer_over at o = 255, no twin involved"""
    import torch
    images, layer = noise
    image = images[300]
    for colour in ((17, 250, 3, 255), (200, 90, 20, 141)):
        got = _paint(ctx, image, layer, (3, 2, 290, 35), (5, 3), (pr.LINEAR, pr.PAD, (0, 0, 640, 0), [(0, colour)]))
        src = torch.from_numpy(layer).to("cuda:0")
        tinted = torch.zeros((35, 290, 4), dtype=torch.uint8, device="cuda:0")
        dst = torch.from_numpy(image.copy()).to("cuda:0")
        torch.cuda.synchronize()
        fr.layer_shadow(ctx, src.data_ptr(), 300, 40, tinted.data_ptr(), 290, 35, (3, 2, 290, 35), (0, 0, 290, 35), (0, 0), 0, 0, 0, colour)
        fr.layer_over(ctx, tinted.data_ptr(), 290, 35, dst.data_ptr(), 300, 40, fr.make_blits([(0, 0, 290, 35, 5, 3, 255)]))
        ctx.sync()
        assert np.array_equal(got, dst.cpu().numpy()) and not np.array_equal(got, image)


def test_consequence_3_a_gradient_text_layer(ctx, noise):
    _, layer = noise
    for srgb in (False, True):
        got = _paint(ctx, np.zeros((40, 300, 4), np.uint8), layer, (0, 0, 300, 40), (0, 0), (pr.RADIAL, pr.REFLECT, (64 * 150, 64 * 20, 64 * 60, 0), CLEAR), srgb).astype(np.int64)
        assert np.array_equal(got[layer[..., 3] == 0], np.zeros_like(got[layer[..., 3] == 0])) and got[..., 3].max() == 255
        if not srgb:
            assert (got[..., :3] <= got[..., 3:]).all()        # valid premultiplied UNORM pixels


# ---- far pixels: a 2-row image in rows of 2^20 + 300 pixels --------------------------------------------------------------
FAR = (1 << 20) + 300


@pytest.fixture(scope="module")
def far():
    """the image (the last 600 columns noise, so the twin's rectangle is not all zero) and a 300 x 2 layer"""
    rng = np.random.default_rng(43)
    image = np.zeros((2, FAR, 4), np.uint8)
    image[:, -600:] = premultiplied(rng, (2, 600))
    return image, premultiplied(rng, (2, 300))


def _d2(grad, X, Y):
    return (64 * X + 32 - grad[2][0]) ** 2 + (64 * Y + 32 - grad[2][1]) ** 2


def test_far_pixels_linear(ctx, far):
    """the last 300 columns, a gradient one pixel long (TX = 2^32): X TX reaches 2^52"""
    image, layer = far
    grad = (pr.LINEAR, pr.REPEAT, (0, 0, 64, 0), STEEP)
    assert pr.linear_coefficients(0, 0, 64, 0)[1] == 1 << 32
    _check(ctx, image, layer, (0, 0, 300, 2), (1 << 20, 0), grad)
    _check(ctx, image, None, (0, 0, 300, 2), (1 << 20, 0), (pr.LINEAR, pr.REFLECT, ((1 << 26) - 700, 7, 1 << 26, 307), STEEP), True)


def _triple_at_the_limit():
    """(X, b): a column X in [2^20 - 300, 2^20) whose ddx = 64 X + 32 + 2^26 from a centre at x0 = -2^26 is a leg of a
    Pythagorean triple (ddx, b, h) with 0 < b <= 2^26 a multiple of 32: ddx = 32 d s and b = 32 (s^2 - d^2) / 2 for odd d < s"""
    for X in range((1 << 20) - 1, (1 << 20) - 301, -1):
        m = (64 * X + 32 + (1 << 26)) // 32
        for d in range(1611, 2048, 2):
            if m % d == 0:
                s = m // d
                b = 16 * (s * s - d * d)
                if s > d and 0 < b <= 1 << 26:
                    return X, b
    raise AssertionError("no triple in range")


def test_far_pixels_radial(ctx, far):
    """The 300 columns that end at column 2^20 - 1, the last whose ddx from a centre at x0 = -2^26 stays below 2^27 (the
    columns from 2^20 on are refused, see test_refusals), with r = 64 and the steep table: s R needs its high 64 bits, and
    a root that is off by one moves the pixel to the next table entry.  (ddx^2 + ddy^2) 256 is a perfect square k^2 on
    the whole of row 0 (ddy = 0), at one pixel of a true Pythagorean triple, and lies just past a square, (h^2 + 1) 256,
    on the whole of row 0 (ddy = 1), and just short of one, (h^2 - 1) 256, at the pixel with (ddx, ddy) = (2 n, 2 n^2),
    h = 2 n^2 + 1: there isqrt is 16 h - 1 and a root rounded to nearest is 16 h."""
    image, layer = far
    left = (1 << 20) - 300
    X, b = _triple_at_the_limit()
    n = 5000
    grads = {"squares_on_row_0": (pr.RADIAL, pr.REPEAT, (-(1 << 26), 32, 64, 0), STEEP),
             "a_triple": (pr.RADIAL, pr.REPEAT, (-(1 << 26), 32 - b, 64, 0), STEEP),
             "just_past_squares_on_row_0": (pr.RADIAL, pr.REPEAT, (-(1 << 26), 31, 64, 0), STEEP),
             "just_short_of_a_square": (pr.RADIAL, pr.REFLECT, (64 * (left + 100) + 32 - 2 * n, 32 - 2 * n * n, 64, 0), STEEP)}
    for Xc in range(left, 1 << 20):
        assert math.isqrt(_d2(grads["squares_on_row_0"], Xc, 0)) ** 2 == _d2(grads["squares_on_row_0"], Xc, 0)
        h = 64 * Xc + 32 + (1 << 26)
        assert _d2(grads["just_past_squares_on_row_0"], Xc, 0) == h * h + 1 and math.isqrt(256 * (h * h + 1)) == 16 * h
    assert 64 * ((1 << 20) - 1) + 32 + (1 << 26) == (1 << 27) - 32 and math.isqrt(_d2(grads["a_triple"], X, 0)) ** 2 == _d2(grads["a_triple"], X, 0) and b > 0
    h = 2 * n * n + 1
    assert _d2(grads["just_short_of_a_square"], left + 100, 0) == h * h - 1 and math.isqrt(256 * (h * h - 1)) == 16 * h - 1
    d = Guarded(image, layer)
    want = image
    for name, grad in grads.items():
        _call(ctx, d, image, layer, (0, 0, 300, 2), (left, 0), grad, name == "a_triple")
        got = d.result(ctx)
        want = pr.paint(want, layer, (0, 0, 300, 2), (left, 0), grad, name == "a_triple")
        assert np.array_equal(got, want), (name, np.argwhere(got != want)[:4])
    assert not np.array_equal(want, image)
    # through full coverage every pixel shows its table entry: u >> 6 = s mod 1024 with r = 64 and FR_SPREAD_REPEAT
    full = _check(ctx, image, None, (0, 0, 300, 2), (left, 0), grads["just_past_squares_on_row_0"])
    G = pr.table(STEEP)
    assert all(tuple(full[0, Xc]) == tuple(G[(16 * (64 * Xc + 32 + (1 << 26))) % 1024]) for Xc in range(left, 1 << 20))


# ---- text ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("srgb", [False, True], ids=["unorm", "srgb"])
def test_a_real_line(ctx, srgb):
    """an FR_TEXT_OVER layer of a DejaVuSans line painted with a three-stop gradient over a frame == the twin, and the frame's
    own bytes wherever the layer's alpha is 0"""
    from font_renderer_amd.text import render_text_rgba
    font = load_font("DejaVuSans.ttf", allow_hinted=True)
    text = render_text_rgba(font, "Gradient quay, fjord", 32, color=(255, 255, 255, 255), over=True, srgb=srgb, ctx=ctx)
    layer = text.as_3d()
    h, w = layer.shape[:2]
    assert layer[..., 3].max() == 255 and (layer[..., 3] == 0).mean() > 0.5 and ((layer[..., 3] > 0) & (layer[..., 3] < 255)).any()
    frame = premultiplied(np.random.default_rng(44), (h + 9, w + 14))
    grad = (pr.LINEAR, pr.PAD, (64 * 7, 64 * 4, 64 * (7 + w), 64 * (4 + h)), [(0, (255, 60, 0, 255)), (30000, (255, 230, 0, 255)), (65536, (0, 120, 255, 200))])
    got = _check(ctx, frame, layer, (0, 0, w, h), (7, 4), grad, srgb)
    empty = np.ones(frame.shape[:2], bool)
    empty[4:4 + h, 7:7 + w] = layer[..., 3] == 0
    assert np.array_equal(got[empty], frame[empty]) and (got[~empty] != frame[~empty]).any()
    # the same through RGBA.paint
    im = fr.RGBA(frame.shape[1], frame.shape[0], frame.reshape(-1, 4).copy())
    assert im.paint(_params(grad), text, 7, 4, srgb=srgb, ctx=ctx) is im and np.array_equal(im.as_3d(), got)


def test_rgba_paint_panel(ctx, noise):
    images, _ = noise
    image = images[300]
    grad = (pr.RADIAL, pr.REFLECT, (64 * 100, 64 * 10, 64 * 25, 0), CLEAR)
    im = fr.RGBA(300, 40, image.reshape(-1, 4).copy()).paint(_params(grad), srgb=True, ctx=ctx)
    assert np.array_equal(im.as_3d(), pr.paint(image, None, (0, 0, 300, 40), (0, 0), grad, True))


def test_stream_order(ctx):
    """render a text layer, paint a gradient through it into a cleared layer and composite that over a frame: one sync at
    the end gives the bytes of a sync after every call"""
    import torch
    from font_renderer_amd.text import _line
    font = load_font("DejaVuSans.ttf", allow_hinted=True)
    gs, places, runs, w, h = _line(font, "Stream order", 24)
    cols = np.full((len(places), 4), 255, np.uint8)
    frame = premultiplied(np.random.default_rng(45), (h, w))
    grad = _params((pr.LINEAR, pr.REFLECT, (0, 0, 64 * 40, 64 * 9), STEEP))
    dgs = fr.DeviceGlyphSet(ctx, gs)
    out = []
    try:
        plan = fr.TextPlanRGBA(dgs, places, cols, runs, [(0, 0, 0, 0)], 4, fr.FR_SAMPLE_CENTER, fr.FR_TEXT_OVER)
        for step in (False, True):
            text = torch.full((h, w, 4), SENT, dtype=torch.uint8, device="cuda:0")
            filled = torch.zeros((h, w, 4), dtype=torch.uint8, device="cuda:0")
            dst = torch.from_numpy(frame.copy()).to("cuda:0")
            torch.cuda.synchronize()
            plan.render(text.data_ptr(), w, h)
            if step:
                ctx.sync()
            fr.layer_paint(ctx, text.data_ptr(), w, h, filled.data_ptr(), w, h, grad, (0, 0, w, h), (0, 0))
            if step:
                ctx.sync()
            fr.layer_over(ctx, filled.data_ptr(), w, h, dst.data_ptr(), w, h, fr.make_blits([(0, 0, w, h, 0, 0, 255)]))
            ctx.sync()
            out.append((text.cpu().numpy(), filled.cpu().numpy(), dst.cpu().numpy()))
        plan.close()
    finally:
        dgs.close()
    assert all(np.array_equal(a, b) for a, b in zip(*out))
    text, filled, dst = out[0]
    assert np.array_equal(filled, pr.paint(np.zeros_like(frame), text, (0, 0, w, h), (0, 0), (pr.LINEAR, pr.REFLECT, (0, 0, 64 * 40, 64 * 9), STEEP)))
    assert not np.array_equal(dst, frame) and filled[..., 3].max() == 255


def test_refusals(ctx, noise):
    import torch
    images, layer = noise
    image = images[300]
    dst, src = torch.from_numpy(image.copy()).to("cuda:0"), torch.from_numpy(layer).to("cuda:0")
    torch.cuda.synchronize()
    D, S = dst.data_ptr(), src.data_ptr()
    lin, rad = fr.make_gradient_linear(0, 0, 6400, 0, TWO), fr.make_gradient_radial(-(1 << 26), 0, 64, TWO)
    win = (0, 0, 300, 40)
    for what, code, call in (
            ("dst NULL", -1, lambda: fr.layer_paint(ctx, S, 300, 40, 0, 300, 40, lin, win)),
            ("dst not 4-byte aligned", -1, lambda: fr.layer_paint(ctx, S, 300, 40, D + 2, 300, 39, lin, win)),
            ("src not 4-byte aligned", -1, lambda: fr.layer_paint(ctx, S + 1, 300, 39, D, 300, 40, lin, win)),
            ("no layer but a stride", -1, lambda: fr.layer_paint(ctx, None, 300, 0, D, 300, 40, lin, win)),
            ("no layer but a window position", -1, lambda: fr.layer_paint(ctx, None, 0, 0, D, 300, 40, lin, (1, 0, 299, 40))),
            ("2^31 rows", -4, lambda: fr.layer_paint(ctx, S, 300, 40, D, 0, 1 << 31, lin, win)),
            ("NULL paint", -1, lambda: fr.layer_paint(ctx, S, 300, 40, D, 300, 40, None, win)),
            ("window leaves the layer", -1, lambda: fr.layer_paint(ctx, S, 300, 40, D, 300, 40, lin, (1, 0, 300, 40))),
            ("the images overlap", -1, lambda: fr.layer_paint(ctx, D + 4 * 300 * 20, 300, 20, D, 300, 40, lin, (0, 0, 300, 20))),
            ("unknown flag", -1, lambda: fr.layer_paint(ctx, S, 300, 40, D, 300, 40, lin, win, flags=2)),
            ("text flag", -1, lambda: fr.layer_paint(ctx, S, 300, 40, D, 300, 40, lin, win, flags=fr.FR_TEXT_OVER)),
            ("decreasing offsets", -1, lambda: fr.layer_paint(ctx, S, 300, 40, D, 300, 40, fr.make_gradient_linear(0, 0, 6400, 0, [(9, (1, 2, 3, 4)), (8, (1, 2, 3, 4))]), win)),
            ("length 0", -1, lambda: fr.layer_paint(ctx, S, 300, 40, D, 300, 40, fr.make_gradient_linear(5, 5, 5, 5, TWO), win)),
            ("radius 0", -1, lambda: fr.layer_paint(ctx, S, 300, 40, D, 300, 40, fr.make_gradient_radial(5, 5, 0, TWO), win)),
            ("under a pixel", -4, lambda: fr.layer_paint(ctx, S, 300, 40, D, 300, 40, fr.make_gradient_radial(5, 5, 63, TWO), win)),
            ("geometry beyond 2^26", -4, lambda: fr.layer_paint(ctx, S, 300, 40, D, 300, 40, fr.make_gradient_linear(0, 0, (1 << 26) + 1, 0, TWO), win)),
            # column 2^20 is 2^27 + 32 sixty-fourths from a centre at -2^26: the rectangle may end at column 2^20 - 1
            ("a corner too far from the centre", -4, lambda: fr.layer_paint(ctx, None, 0, 0, D, FAR, 2, rad, (0, 0, 300, 2), (1 << 20, 0)))):
        with pytest.raises(fr.FrError) as e:
            call()
        assert e.value.code == code, what
    bad = L.LayerPaintParams.from_buffer_copy(lin)
    bad.kind = 2
    lib = L.load_library()
    assert lib.fr_layer_paint(ctx._h, S, 300, 40, D, 300, 40, bad, 0) == -1 and lib.fr_layer_paint(None, S, 300, 40, D, 300, 40, lin, 0) == -1
    with pytest.raises(ValueError):
        fr.make_gradient_linear(0, 0, 6400, 0, [])
    with pytest.raises(ValueError):
        fr.make_gradient_radial(0, 0, 6400, [(0, (1, 2, 3, 256))])
    ctx.sync()
    assert np.array_equal(dst.cpu().numpy(), image) and np.array_equal(src.cpu().numpy(), layer)

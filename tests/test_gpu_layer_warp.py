"""fr_layer_warp on the GPU (include/fr_raster.h).  The expected image never comes from the code under test: it is the numpy
twin of the definition (tests/layer_warp_ref.py, itself held to a brute force and to the header's consequences by
tests/test_layer_warp_ref.py), or the device's own fr_layer_over where a consequence names it.  Every comparison is byte for
byte.  Destinations are noise with guard rows around them, and whole arrays are compared, so a byte written outside a
clipped rectangle fails; the layer is compared with its copy afterwards."""
import math

import numpy as np
import pytest

import font_renderer_amd as fr
import layer_ref as lr
import layer_shadow_ref as sr
import layer_warp_ref as wr
import text_gpu as tg
from fixtures import load_font
from font_renderer_amd import _lib as L
from layer_gpu import SENT, Guarded, premultiplied

pytestmark = pytest.mark.gpu
SPACES = pytest.mark.parametrize("srgb", [False, True], ids=["unorm", "srgb"])
ONE, HALF = wr.ONE, wr.HALF
I31 = 2 ** 31 - 1


def _run(ctx, layer, image, blits, srgb=False, dst_skip=0, src_skip=0):
    """fr_layer_warp of `layer` over a guarded device copy of `image` -> the image after; the layer is checked against its copy"""
    d = Guarded(image, layer, dst_skip, src_skip)
    fr.layer_warp(ctx, d.src, layer.shape[1], layer.shape[0], d.dst, image.shape[1], image.shape[0], fr.make_warp_blits(blits), srgb)
    return d.result(ctx)


def _check(ctx, layer, image, blits, srgb=False, **skips):
    got = _run(ctx, layer, image, blits, srgb, **skips)
    want = wr.composite(layer, image, blits, srgb)
    assert np.array_equal(got, want), (blits[:2], skips, np.argwhere(got != want)[:4])
    return got


def _device_over(ctx, layer, image, rows, srgb):
    """the device's fr_layer_over on a guarded copy of image"""
    d = Guarded(image, layer)
    fr.layer_over(ctx, d.src, layer.shape[1], layer.shape[0], d.dst, image.shape[1], image.shape[0], fr.make_blits(rows), srgb)
    return d.result(ctx)


def _placed(angle, scale, window, centre, opacity=255):
    """the window turned by `angle` degrees and scaled about its centre, that centre landing on `centre` of the image"""
    c, s = scale * math.cos(math.radians(angle)), scale * math.sin(math.radians(angle))
    mx, my = window[2] / 2, window[3] / 2
    return fr.warp_from_matrix(((c, -s, centre[0] - c * mx + s * my), (s, c, centre[1] - s * mx - c * my)), window, opacity)


@pytest.fixture(scope="module")
def scene():
    rng = np.random.default_rng(41)
    return premultiplied(rng, (50, 70)), premultiplied(rng, (200, 300))


# ---- every instance, at every angle and scale ---------------------------------------------------------------------------------
@SPACES
@pytest.mark.parametrize("scale", [0.4, 1, 2.5])
@pytest.mark.parametrize("angle", [0, 5, 30, 45, 90])
def test_every_instance(ctx, scene, srgb, angle, scale):
    """the whole 70 x 50 layer turned and scaled about the middle of a 300 x 200 image, at o = 255 (OPACITY = 0) and at 128
    and 1 (OPACITY = 1), on image rows on and off the 16-byte grid (tests/test_layer_warp_tables.py: the vector flag)"""
    layer, image = scene
    for o, skip in ((255, 0), (128, 1), (1, 0), (255, 3)):
        got = _check(ctx, layer, image, [_placed(angle, scale, (0, 0, 70, 50), (150.25, 99.5), o)], srgb, dst_skip=skip, src_skip=skip)
        assert not np.array_equal(got, image)


# ---- the consequences that name fr_layer_over, against that call on the device ------------------------------------------------
@SPACES
def test_consequence_1_against_fr_layer_over(ctx, scene, srgb):
    """a 37 x 21 window at every dst_x mod 4, across the tile border at 32 and 64; then a rectangle inside the window, moved"""
    layer, image = scene
    for o in (255, 128):
        for dx in (28, 29, 30, 31):
            got = _run(ctx, layer, image, [wr.identity((9, 11, 37, 21), (dx, 25), o)], srgb)
            want = _device_over(ctx, layer, image, [(9, 11, 37, 21, dx, 25, o)], srgb)
            assert np.array_equal(got, want) and not np.array_equal(got, image), (o, dx)
    blit = wr.identity((9, 11, 37, 21), (-4, 190), 77, 3, 2)
    got = _run(ctx, layer, image, [blit[:6] + (30, 15) + blit[8:]], srgb)
    assert np.array_equal(got, _device_over(ctx, layer, image, [(12, 13, 30, 15, -4, 190, 77)], srgb))


@SPACES
def test_consequence_2_the_eight_symmetries(ctx, scene, srgb):
    layer, image = scene
    for name, (turn, coeff) in wr.symmetries(70, 50).items():
        turned = np.ascontiguousarray(turn(layer))
        th, tw = turned.shape[:2]
        got = _run(ctx, layer, image, [(0, 0, 70, 50, 45, 61, tw, th) + coeff + (200,)], srgb)
        assert np.array_equal(got, _device_over(ctx, turned, image, [(0, 0, tw, th, 45, 61, 200)], srgb)), name


# ---- the arithmetic over its domain -------------------------------------------------------------------------------------------
@SPACES
@pytest.mark.parametrize("axis", ["horizontal", "vertical"])
def test_every_pair_at_every_fraction(ctx, srgb, axis):
    """every (p, q, f) of one step: blit p samples between a pixel whose four bytes are p and pixels whose bytes carry four
    different q, 64 pairs across (ux = 131072 skips from pair to pair), f down the 256 rows (uy or vy = 256); 256 stacked
    blits in one call at o = 255 over a cleared image, so that the output is the sample (UNORM) or E of it"""
    q = np.arange(256, dtype=np.uint8).reshape(64, 4)
    if axis == "horizontal":
        layer = np.empty((256, 128, 4), np.uint8)
        layer[:, 0::2], layer[:, 1::2] = np.arange(256, dtype=np.uint8)[:, None, None], q[None]
        blits = [(0, p, 128, 1, 0, 256 * p, 64, 256, HALF, HALF, 2 * ONE, 256, 0, 0, 255) for p in range(256)]
    else:
        layer = np.empty((512, 64, 4), np.uint8)
        layer[0::2], layer[1::2] = np.arange(256, dtype=np.uint8)[:, None, None], q[None]
        blits = [(0, 2 * p, 64, 2, 0, 256 * p, 64, 256, HALF, HALF, ONE, 0, 0, 256, 255) for p in range(256)]
    image = np.zeros((65536, 64, 4), np.uint8)
    got = _check(ctx, layer, image, blits, srgb)
    if not srgb:                                                # the sample itself: row f of blit p, pair k, byte c
        p, f = np.arange(256)[:, None, None, None], np.arange(256)[None, :, None, None]
        assert np.array_equal(got.reshape(256, 256, 64, 4), (p * (256 - f) * 256 + q.astype(np.int64)[None, None] * f * 256 + 32768) >> 16)


@SPACES
def test_every_fx_and_fy(ctx, srgb):
    """a 2 x 2 window of four different pixels with ux = vy = 256: pixel (X, Y) has fx = X, fy = Y"""
    layer = np.array([[(10, 20, 30, 40), (250, 128, 0, 255)], [(0, 0, 0, 0), (77, 200, 199, 201)]], np.uint8)
    image = premultiplied(np.random.default_rng(2), (256, 256))
    for o in (255, 100):
        _check(ctx, layer, image, [(0, 0, 2, 2, 0, 0, 256, 256, HALF, HALF, 256, 0, 0, 256, o)], srgb)


# ---- the window's edges ---------------------------------------------------------------------------------------------------------
@SPACES
@pytest.mark.parametrize("window", [(1, 1), (1, 9), (9, 1), (9, 9)], ids=lambda w: "%dx%d" % w)
def test_window_edges(ctx, srgb, window):
    """the window inside a layer whose other pixels are all 255: moved by 1/4, 1/2 and 255/256 of a pixel in each direction,
    its rim blends with zero and never with the 255 around it"""
    w, h = window
    rng = np.random.default_rng(5)
    layer = np.full((16, 20, 4), 255, np.uint8)
    layer[4:4 + h, 6:6 + w] = premultiplied(rng, (h, w))
    layer[4, 6] = (200, 100, 50, 255)
    image = premultiplied(rng, (40, 52))
    blits = []
    for k, (fx, fy) in enumerate((a * s, b * s) for s in (ONE // 4, ONE // 2, ONE * 255 // 256) for a, b in ((1, 0), (-1, 0), (0, 1), (0, -1), (1, 1), (-1, -1))):
        # a 13 x 13 rectangle around the window (two more pixels on every side): twelve on a grid, then six more on a second image
        blits.append((6, 4, w, h, 13 * (k % 4), 13 * (k % 12 // 4), 13, 13, HALF - 2 * ONE + fx, HALF - 2 * ONE + fy, ONE, 0, 0, ONE, 255 if k % 2 else 180))
    got = _check(ctx, layer, image, blits[:12], srgb)
    bare = np.zeros_like(layer)
    bare[4:4 + h, 6:6 + w] = layer[4:4 + h, 6:6 + w]
    assert np.array_equal(_run(ctx, bare, image, blits[:12], srgb), got) and not np.array_equal(got, image)
    image2 = premultiplied(rng, (26, 52))
    assert np.array_equal(_check(ctx, layer, image2, blits[12:], srgb), _run(ctx, bare, image2, blits[12:], srgb))


# ---- extremes ---------------------------------------------------------------------------------------------------------------
@SPACES
def test_extreme_coefficients_and_origins(ctx, scene, srgb):
    layer, image = scene
    for c in (I31, -I31, -2 ** 31):                                          # one pixel samples the window, its neighbours are far away
        for u0, v0 in ((HALF + 20 * ONE + 9000, HALF + 30 * ONE + 77), (69 * ONE, 49 * ONE)):
            got = _check(ctx, layer, image, [(0, 0, 70, 50, 7, 5, 290, 190, u0, v0, c, -c if c != -2 ** 31 else c, c, c, 255)], srgb)
            assert not np.array_equal(got[5, 7], image[5, 7]) and (got != image).any(axis=2).sum() == 1
    # u0 = -2^47 at 2^30 a column: column 2^17 samples U = 0, half of window column 0, rows 20 .. 22
    wide = premultiplied(np.random.default_rng(6), (3, 2 ** 17 + 4))
    got = _check(ctx, layer, wide, [(0, 0, 70, 50, 0, 0, 2 ** 17 + 4, 3, -2 ** 47, HALF + 20 * ONE, 2 ** 30, 0, 0, ONE, 255)], srgb)
    assert (got != wide).any(axis=2).nonzero()[1].tolist() == [2 ** 17] * 3
    _check(ctx, layer, wide, [(0, 0, 70, 50, 4, 0, 2 ** 17, 3, 2 ** 47, -2 ** 47, -2 ** 30, 1, 0, I31, 255)], srgb)      # U stops 2^30 short of the window, V is never near
    tall = premultiplied(np.random.default_rng(7), (300, 8))
    got = _check(ctx, layer, tall, [(0, 0, 70, 50, 1, 0, 5, 300, 3 * ONE, 2 ** 47, 0, 0, 0, -I31, 128)], srgb, dst_skip=2)
    assert np.array_equal(got, tall)                                            # 2^47 / (2^31 - 1) rows is beyond the image
    # the zero matrix: every pixel samples one point
    got = _check(ctx, layer, image, [(0, 0, 70, 50, 33, 31, 70, 40, 5 * ONE + 77, 6 * ONE + 40000, 0, 0, 0, 0, 255)], srgb)
    assert not np.array_equal(got[31:71, 33:103], image[31:71, 33:103])
    assert np.array_equal(_check(ctx, layer, image, [(0, 0, 70, 50, 33, 31, 70, 40, -HALF - 1, 6 * ONE, 0, 0, 0, 0, 255)], srgb), image)


@SPACES
def test_large_rectangles_and_rectangles_nothing_reaches(ctx, scene, srgb):
    layer, image = scene
    # 2^20 x 2^20 around an 8 x 8 window, clipped by the image: the host lists one tile (tests/test_layer_warp_tables.py)
    big = (20, 20, 8, 8, -2 ** 19, -2 ** 19, 2 ** 20, 2 ** 20, HALF - (2 ** 19 + 150) * ONE, HALF - (2 ** 19 + 100) * ONE, ONE, 0, 0, ONE, 255)
    got = _check(ctx, layer, image, [big], srgb)
    assert np.array_equal(got[100:108, 150:158], lr.over(layer[20:28, 20:28], image[100:108, 150:158], 255, srgb))
    r = _placed(30, 3.0, (20, 20, 8, 8), (150.3, 99.9), 200)                # the same map from a corner 2^19 pixels up and to the left
    X, Y = r[4] + 2 ** 19, r[5] + 2 ** 19
    turned = r[:4] + (-2 ** 19, -2 ** 19, 2 ** 20, 2 ** 20, r[8] - X * r[10] - Y * r[11], r[9] - X * r[12] - Y * r[13]) + r[10:]
    assert not np.array_equal(_check(ctx, layer, image, [turned], srgb), image)
    # wholly off the image; no tap reaches the window; an empty window; o = 0: nothing is launched, nothing changes
    for blit in ((0, 0, 70, 50, 300, 0, 70, 50, HALF, HALF, ONE, 0, 0, ONE, 255), (0, 0, 70, 50, -70, -50, 70, 50, HALF, HALF, ONE, 0, 0, ONE, 255),
                 (0, 0, 70, 50, 0, 0, 300, 200, HALF + 71 * ONE, HALF, ONE, 0, 0, ONE, 255), (5, 5, 0, 9, 0, 0, 300, 200, HALF, HALF, ONE, 0, 0, ONE, 255),
                 (0, 0, 70, 50, 10, 10, 70, 50, HALF, HALF, ONE, 0, 0, ONE, 0), (0, 0, 70, 50, 10, 10, 0, 50, HALF, HALF, ONE, 0, 0, ONE, 255)):
        assert np.array_equal(_check(ctx, layer, image, [blit], srgb), image), blit


@SPACES
def test_touching_rectangles_and_tile_borders(ctx, scene, srgb):
    """rectangles that touch, each with its own map and opacity, in one call; one of them crosses tile borders both ways"""
    layer, image = scene
    c = round(ONE * math.cos(math.radians(45)))
    blits = [
        (0, 0, 70, 50, 17, 13, 100, 100, -20 * ONE, 25 * ONE, c, c, -c, c, 255),                 # four tiles by four
        (0, 0, 70, 50, 117, 13, 60, 60, HALF, HALF, ONE, 0, 0, ONE, 128),
        (5, 5, 30, 30, 17, 113, 160, 33, 0, 0, ONE // 4, 0, 0, ONE, 1),
        (0, 0, 70, 50, 177, 13, 33, 93, HALF + 69 * ONE, HALF, -ONE, 0, 0, ONE // 2, 77),
        (10, 10, 40, 30, -9, 146, 309, 54, -3 * ONE, -2 * ONE, 9000, 100, -50, 40000, 200),      # clipped on three sides
    ]
    for skip in (0, 1):
        got = _check(ctx, layer, image, blits, srgb, dst_skip=skip)
        for b in blits:
            assert not np.array_equal(got[max(b[5], 0):b[5] + b[7], max(b[4], 0):b[4] + b[6]], image[max(b[5], 0):b[5] + b[7], max(b[4], 0):b[4] + b[6]]), b


# ---- the interface ------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_image_untouched(ctx, scene):
    """every refusal of the header through the C ABI: its code, and not a byte of the image or the layer changed"""
    import torch
    layer = scene[0]
    image = np.full((200, 300, 4), SENT, np.uint8)
    src, dst = (torch.from_numpy(a.copy()).to("cuda:0") for a in (layer, image))
    torch.cuda.synchronize()
    S, D = src.data_ptr(), dst.data_ptr()
    ok = (0, 0, 70, 50, 0, 0, 70, 50, HALF, HALF, ONE, 0, 0, ONE, 255)

    def call(s=S, ss=70, srows=50, d=D, ds=300, dr=200, rows=(ok,), **kw):
        fr.layer_warp(ctx, s, ss, srows, d, ds, dr, fr.make_warp_blits(rows), **kw)

    def but(**kw):
        row = dict(zip(wr.FIELDS, ok), **kw)
        return [tuple(row[f] for f in wr.FIELDS) + ((row["reserved"],) if "reserved" in row else ())]

    cases = {
        "opacity 256": (-1, dict(rows=but(opacity=256))),
        "reserved 1": (-1, dict(rows=but(reserved=1))),
        "u0 above 2^47": (-1, dict(rows=but(u0=2 ** 47 + 1))),
        "v0 below -2^47": (-1, dict(rows=but(v0=-2 ** 47 - 1))),
        "dst_w above 2^26": (-1, dict(rows=but(dst_w=2 ** 26 + 1))),
        "dst_h above 2^26": (-1, dict(rows=but(dst_h=2 ** 26 + 1))),
        "the window one pixel out of the layer": (-1, dict(rows=but(src_x=1))),
        "the window one row out of the layer": (-1, dict(rows=but(src_y=1))),
        "rectangles overlap by one pixel": (-1, dict(rows=but(dst_w=20, dst_h=10) + but(dst_x=19, dst_y=9, opacity=0))),
        "the image is the layer": (-1, dict(s=D, ss=300, srows=200)),
        "src not 4-byte aligned": (-1, dict(s=S + 2, srows=49)),
        "dst not 4-byte aligned": (-1, dict(d=D + 1, dr=199)),
        "src NULL": (-1, dict(s=0)),
        "dst NULL": (-1, dict(d=0)),
        "dst pitch beyond 2^26": (-1, dict(ds=(1 << 26) + 1, dr=0)),
        "src pitch beyond 2^26": (-1, dict(ss=(1 << 26) + 1, srows=0, rows=but(w=0, h=0))),
        "2^31 rows of image": (-4, dict(ds=0, dr=1 << 31)),
        "2^31 rows of layer": (-4, dict(ss=0, srows=1 << 31)),
        "more than 2^22 tiles": (-4, dict(d=1 << 40, ds=1 << 26, dr=1 << 11, rows=but(dst_w=1 << 26, dst_h=1 << 11))),     # refused before any memory is touched
    }
    for what, (code, kw) in cases.items():
        with pytest.raises(fr.FrError) as e:
            call(**kw)
        assert e.value.code == code, (what, str(e.value))
    for flags in (fr.FR_LCD_BGR, fr.FR_MASK_PLANE, fr.FR_MASK_ERASE, 16, fr.FR_TEXT_OVER, 1 << 31):
        with pytest.raises(fr.FrError) as e:
            call(flags=flags)
        assert e.value.code == -1, flags
    lib = L.load_library()
    with pytest.raises(fr.FrError) as e:                               # NULL blits with a count
        L.check(lib.fr_layer_warp(ctx._h, S, 70, 50, D, 300, 200, None, 1, 0))
    assert e.value.code == -1
    with pytest.raises(fr.FrError) as e:                               # NULL ctx
        L.check(lib.fr_layer_warp(None, S, 70, 50, D, 300, 200, None, 0, 0))
    assert e.value.code == -1
    fr.layer_warp(ctx, S, 70, 50, D, 300, 200, None)                   # no blits: valid
    ctx.sync()
    assert np.array_equal(dst.cpu().numpy(), image) and np.array_equal(src.cpu().numpy(), layer)
    call()                                                             # and the call still works
    ctx.sync()
    assert np.array_equal(dst.cpu().numpy(), wr.composite(layer, image, [ok]))


# ---- end to end: a real font, one stream, no sync between the calls ------------------------------------------------------------
def _text_scene(ctx, srgb, text, frame_shape):
    """a DejaVuSans line as a plan that renders a premultiplied layer, and device buffers: the layer, two scratch layers of
    the frame's size and a noise frame of frame_shape(w, h) = (rows, pixels)"""
    import torch
    from font_renderer_amd.text import _line
    font = load_font("DejaVuSans.ttf", allow_hinted=True)
    gs, places, runs, w, h = _line(font, text, 19)
    cols = tg.colours(len(places), 5, opaque=True)
    dgs = fr.DeviceGlyphSet(ctx, gs)
    plan = fr.TextPlanRGBA(dgs, places, cols, runs, [(0, 0, 0, 0)], 1, fr.FR_SAMPLE_CENTER, fr.FR_TEXT_OVER | (fr.FR_TEXT_SRGB if srgb else 0))
    H, W = frame_shape(w, h)
    frame = tg.noise((H, W), 9)
    dev = {"text": torch.zeros((h, w, 4), dtype=torch.uint8, device="cuda:0"), "a": torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda:0"),
           "b": torch.full((H, W, 4), SENT, dtype=torch.uint8, device="cuda:0"), "frame": torch.from_numpy(frame.copy()).to("cuda:0")}
    torch.cuda.synchronize()
    return dgs, plan, dev, frame, (w, h)


@SPACES
def test_a_real_font_line_zoomed_and_turned(ctx, srgb):
    """the line rendered as an FR_TEXT_OVER layer, then zoomed by 2 and turned by 10 degrees over a noise frame, against the
    twin on the layer read back; then render and warp issued with no sync between them: stream order"""
    dgs, plan, dev, frame, (w, h) = _text_scene(ctx, srgb, "Warped fjord quay", lambda w, h: (6 * h, (2 * w + 40) // 4 * 4))
    H, W = frame.shape[:2]
    zoom = fr.warp_from_matrix(((2, 0, 10.5), (0, 2, 20.25)), (0, 0, w, h), 255)
    turn = _placed(10, 1.0, (0, 0, w, h), (W / 2, H / 2), 200)
    try:
        plan.render(dev["text"].data_ptr(), w, h)
        ctx.sync()
        text = dev["text"].cpu().numpy()
        assert text[..., 3].max() == 255 and (text[..., 3] == 0).any()
        fr.layer_warp(ctx, dev["text"].data_ptr(), w, h, dev["frame"].data_ptr(), W, H, fr.make_warp_blits([zoom]), srgb)
        ctx.sync()
        got = dev["frame"].cpu().numpy()
        want = wr.composite(text, frame, [zoom], srgb)
        assert np.array_equal(got, want) and not np.array_equal(got, frame), np.argwhere(got != want)[:4]
        dev["text"].zero_()
        import torch
        torch.cuda.synchronize()
        plan.render(dev["text"].data_ptr(), w, h)
        fr.layer_warp(ctx, dev["text"].data_ptr(), w, h, dev["frame"].data_ptr(), W, H, fr.make_warp_blits([turn]), srgb)
        ctx.sync()
    finally:
        plan.close()
        dgs.close()
    assert np.array_equal(dev["text"].cpu().numpy(), text)
    got2 = dev["frame"].cpu().numpy()
    want2 = wr.composite(text, want, [turn], srgb)
    assert np.array_equal(got2, want2) and not np.array_equal(got2, want), np.argwhere(got2 != want2)[:4]


@SPACES
def test_the_route_to_a_half_pixel_shadow(ctx, srgb):
    """DESIGN section 9's route: the text layer warped by half a pixel each way into a cleared layer, fr_layer_shadow of that
    layer, composited under the text; four calls behind the render with no sync"""
    pad = 8
    dgs, plan, dev, frame, (w, h) = _text_scene(ctx, srgb, "Soft shadow", lambda w, h: (h + 2 * pad + 5, (w + 2 * pad + 7) // 4 * 4))
    H, W = frame.shape[:2]
    move = fr.warp_from_matrix(((1, 0, pad + 0.5), (0, 1, pad + 0.5)), (0, 0, w, h), 255)
    rgba = (10, 20, 60, 180)
    try:
        plan.render(dev["text"].data_ptr(), w, h)
        fr.layer_warp(ctx, dev["text"].data_ptr(), w, h, dev["a"].data_ptr(), W, H, fr.make_warp_blits([move]), srgb)
        fr.layer_shadow(ctx, dev["a"].data_ptr(), W, H, dev["b"].data_ptr(), W, H, (0, 0, W, H), (0, 0, W, H), (1, 1), 0, 2, 2, rgba, srgb)
        fr.layer_over(ctx, dev["b"].data_ptr(), W, H, dev["frame"].data_ptr(), W, H, fr.make_blits([(0, 0, W, H, 0, 0, 255)]), srgb)
        fr.layer_over(ctx, dev["text"].data_ptr(), w, h, dev["frame"].data_ptr(), W, H, fr.make_blits([(0, 0, w, h, pad, pad, 255)]), srgb)
        ctx.sync()
    finally:
        plan.close()
        dgs.close()
    text = dev["text"].cpu().numpy()
    moved = wr.composite(text, np.zeros((H, W, 4), np.uint8), [move], srgb)
    assert np.array_equal(dev["a"].cpu().numpy(), moved)
    a = text.astype(np.int64)
    assert np.array_equal(moved[pad + 1:pad + h, pad + 1:pad + w, 3], (a[:-1, :-1, 3] + a[:-1, 1:, 3] + a[1:, :-1, 3] + a[1:, 1:, 3] + 2) >> 2)
    shadow = sr.shadow(moved, np.full((H, W, 4), SENT, np.uint8), (0, 0, W, H), (0, 0, W, H), (1, 1), 0, 2, 2, rgba, srgb)
    assert np.array_equal(dev["b"].cpu().numpy(), shadow)
    want = lr.composite(text, lr.composite(shadow, frame, [(0, 0, W, H, 0, 0, 255)], srgb), [(0, 0, w, h, pad, pad, 255)], srgb)
    assert np.array_equal(dev["frame"].cpu().numpy(), want)


def test_rgba_over_warped_method(ctx, scene):
    layer = fr.RGBA(70, 50, scene[0].reshape(-1, 4).copy())
    start = premultiplied(np.random.default_rng(5), (90, 120))
    matrix = ((1.2, -0.5, 30.25), (0.4, 0.9, 10.0))
    for srgb, o in ((False, 255), (True, 77)):
        frame = fr.RGBA(120, 90, start.reshape(-1, 4).copy())
        assert frame.over_warped(layer, matrix, opacity=o, srgb=srgb, ctx=ctx) is frame
        want = wr.composite(scene[0], start, [fr.warp_from_matrix(matrix, (0, 0, 70, 50), o)], srgb)
        assert np.array_equal(frame.as_3d(), want) and not np.array_equal(want, start)
    with pytest.raises(ValueError):
        fr.RGBA(120, 90, start.reshape(-1, 4).copy()).over_warped(layer, matrix, opacity=256, ctx=ctx)

"""fr_layer_shadow on the GPU (include/fr_raster.h).  The expected image never comes from the code under test: it is the
numpy twin of the definition (tests/layer_shadow_ref.py, itself held to a brute-force loop and to the header's consequences
by tests/test_layer_shadow_ref.py).  Destinations are sentinel-filled with guard rows around them, and whole arrays are
compared, so a byte written outside the rectangle fails, and so does an unwritten pixel inside it; the layer is compared
with its copy afterwards."""
import numpy as np
import pytest

import font_renderer_amd as fr
import layer_ref as lr
import layer_shadow_ref as sr
import text_gpu as tg
from fixtures import load_font
from font_renderer_amd import _lib as L
from layer_gpu import SENT, Guarded, premultiplied

pytestmark = pytest.mark.gpu


def _dev(layer, dst_shape, src_skip=0, dst_skip=0):
    """a layer and a sentinel-filled destination on the device, each optionally moved off the 16-byte grid"""
    return Guarded(np.full(dst_shape + (4,), SENT, np.uint8), layer, dst_skip, src_skip)


def _shadow(ctx, d, window, rect, offset, s, r, p, rgba, srgb=False, flags=0):
    fr.layer_shadow(ctx, d.src, d.layer.shape[1], d.layer.shape[0], d.dst, d.image.shape[1], d.image.shape[0], window, rect, offset, s, r, p, rgba, srgb,
                    flags)


def _run(ctx, layer, dst_shape, window, rect, offset, s, r, p, rgba, srgb=False, src_skip=0, dst_skip=0):
    """one call on fresh buffers -> (got, want)"""
    d = _dev(layer, dst_shape, src_skip, dst_skip)
    _shadow(ctx, d, window, rect, offset, s, r, p, rgba, srgb)
    return d.result(ctx), sr.shadow(layer, d.image, window, rect, offset, s, r, p, rgba, srgb)


@pytest.fixture(scope="module")
def layers():
    rng = np.random.default_rng(17)
    return {"small": premultiplied(rng, (41, 97)), "wide": premultiplied(rng, (70, 300))}


# ---- impulses ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r", [1, 2, 3, 7, 16, 32])
def test_impulses(ctx, r):
    """a 1 x 1 window, and a single 255 pixel at each of the four corners and at the centre of a 70 x 40 window (five layers
    of one impulse each), for every p and s; with s = 0 and p = 1 the 1 x 1 window gives consequence 6"""
    one = np.zeros((1, 1, 4), np.uint8)
    one[0, 0, 3] = 255
    singles = []
    for y, x in ((0, 0), (0, 69), (39, 0), (39, 69), (20, 35)):
        singles.append(np.zeros((40, 70, 4), np.uint8))
        singles[-1][y, x] = 255
    for p in (1, 2, 3):
        for s in (0, 1, 3, 8):
            R = s + p * r
            for layer in [one] + singles:
                h, w = layer.shape[:2]
                rows, cols = h + 2 * R + 4, w + 2 * R + 5
                got, want = _run(ctx, layer, (rows, cols), (0, 0, w, h), (1, 1, cols - 2, rows - 2), (R + 1, R + 1), s, r, p, (255, 200, 100, 255))
                assert np.array_equal(got, want), (r, p, s, w, np.argwhere(got != want)[:4])
            if s == 0 and p == 1:
                W = (2 * r + 1) ** 2
                alpha = np.zeros((2 * R + 5, 2 * R + 6), np.uint8)
                alpha[2:2 + 2 * r + 1, 2:2 + 2 * r + 1] = (255 + W // 2) // W
                one_got, _ = _run(ctx, one, (2 * R + 5, 2 * R + 6), (0, 0, 1, 1), (0, 0, 2 * R + 6, 2 * R + 5), (R + 2, R + 2), 0, r, 1, (255, 255, 255, 255))
                assert np.array_equal(one_got[..., 3], alpha)


# ---- tile borders and ragged edges ---------------------------------------------------------------------------------------
STAGES = {"none": (0, 0, 0), "spread2": (2, 0, 0), "box16": (0, 16, 1), "box7x2": (0, 7, 2), "all": (1, 3, 3)}
# (layer, window, dst rows, rect as a function of the reach, offset as a function of the reach)
GEOMETRY = {
    "padded": ("small", (0, 0, 97, 41), lambda R: (1, 2, 97 + 2 * R, 41 + 2 * R), lambda R: (R, R)),
    "unpadded": ("small", (0, 0, 97, 41), lambda R: (5, 3, 97, 41), lambda R: (0, 0)),
    "cut_left_top": ("small", (0, 0, 97, 41), lambda R: (0, 0, 60, 30), lambda R: (-20, -15)),
    "cut_right_bottom": ("small", (0, 0, 97, 41), lambda R: (4, 4, 80, 35), lambda R: (40, 20)),
    "negative_offset": ("small", (0, 0, 97, 41), lambda R: (2, 1, 110, 50), lambda R: (-7, -9)),
    "positive_offset": ("small", (0, 0, 97, 41), lambda R: (2, 1, 110, 50), lambda R: (11, 6)),
    "far_away": ("small", (0, 0, 97, 41), lambda R: (3, 3, 50, 20), lambda R: (-(97 + R), 0)),
    "far_away_up": ("small", (0, 0, 97, 41), lambda R: (3, 3, 50, 20), lambda R: (0, 20 + R)),
    "just_in_reach": ("small", (0, 0, 97, 41), lambda R: (3, 3, 50, 20), lambda R: (-(97 + R - 1), -(41 + R - 1))),
    "window_in_a_wider_layer": ("wide", (101, 13, 120, 40), lambda R: (0, 0, 120 + 2 * R, 40 + 2 * R), lambda R: (R, R)),
    "window_at_the_layers_corner": ("wide", (203, 29, 97, 41), lambda R: (2, 2, 100, 60), lambda R: (1, 5)),
    "three_tiles_wide": ("wide", (0, 0, 300, 70), lambda R: (0, 0, 300 + 2 * R, 70 + 2 * R), lambda R: (R, R)),
}


@pytest.mark.parametrize("stride,src_skip,dst_skip", [(131, 0, 0), (132, 0, 0), (132, 1, 0), (132, 0, 3), (131, 3, 1)],
                         ids=["rows131", "rows132", "src_off_grid_1", "dst_off_grid_3", "both_off_grid"])
@pytest.mark.parametrize("stages", sorted(STAGES))
@pytest.mark.parametrize("case", sorted(GEOMETRY))
def test_geometry(ctx, layers, case, stages, stride, src_skip, dst_skip):
    """random premultiplied layers of 97 x 41 and 300 x 70 into a sentinel-filled destination: rows of 131 take the
    pixel-by-pixel stores, rows of 132 the 16-byte ones with ragged edges"""
    name, window, rect, offset = GEOMETRY[case]
    s, r, p = STAGES[stages]
    R = sr.reach(s, r, p)
    rect, offset = rect(R), offset(R)
    cols = max(stride, rect[0] + rect[2] + 1)
    cols += (stride - cols) % 4                                 # wider where the rectangle needs it, the same residue modulo 4
    for srgb in (False, True):
        got, want = _run(ctx, layers[name], (rect[1] + rect[3] + 2, cols), window, rect, offset, s, r, p, (30, 144, 255, 200), srgb, src_skip, dst_skip)
        assert np.array_equal(got, want), (case, stages, srgb, np.argwhere(got != want)[:4])
    if case in ("far_away", "far_away_up"):
        assert not want[rect[1]:rect[1] + rect[3], rect[0]:rect[0] + rect[2]].any()
    if case == "just_in_reach":
        assert (want[rect[1]:rect[1] + rect[3], rect[0]:rect[0] + rect[2], 3] != 0).sum() <= 1


@pytest.mark.parametrize("dst_w", [1, 3, 63, 64, 65])
@pytest.mark.parametrize("dst_x", [0, 1, 6])
def test_rectangle_widths(ctx, layers, dst_w, dst_x):
    for s, r, p in ((0, 0, 0), (1, 3, 3), (0, 32, 1)):
        got, want = _run(ctx, layers["small"], (50, 132), (0, 0, 97, 41), (dst_x, 2, dst_w, 45), (-17, 3), s, r, p, (255, 0, 128, 255), True)
        assert np.array_equal(got, want), (s, r, p, np.argwhere(got != want)[:4])


def test_zero_sizes(ctx, layers):
    """dst_w or dst_h of 0 writes nothing; a window without area writes zeros over the rectangle"""
    d = _dev(layers["small"], (50, 132))
    _shadow(ctx, d, (0, 0, 97, 41), (7, 7, 0, 30), (0, 0), 1, 3, 3, (1, 2, 3, 255))
    _shadow(ctx, d, (0, 0, 97, 41), (1000, 1000, 30, 0), (0, 0), 1, 3, 3, (1, 2, 3, 255))
    assert np.array_equal(d.result(ctx), d.image)
    _shadow(ctx, d, (500, 500, 0, 41), (7, 8, 90, 30), (0, 0), 1, 3, 3, (1, 2, 3, 255))
    _shadow(ctx, d, (0, 0, 97, 0), (100, 40, 31, 9), (0, 0), 0, 0, 0, (1, 2, 3, 255))
    want = d.image.copy()
    want[8:38, 7:97] = 0
    want[40:49, 100:131] = 0
    assert np.array_equal(d.result(ctx), want)


def test_consequence_1_and_translation(ctx, layers):
    layer = layers["small"]
    got, _ = _run(ctx, layer, (41, 100), (0, 0, 97, 41), (0, 0, 97, 41), (0, 0), 0, 0, 0, (255, 255, 255, 255))
    assert np.array_equal(got[:, :97], np.repeat(layer[..., 3:], 4, -1))
    base, _ = _run(ctx, layer, (80, 132), (0, 0, 97, 41), (0, 0, 132, 80), (12, 12), 1, 3, 2, (200, 100, 50, 220))
    for dx, dy in ((1, 0), (0, 1), (3, 2), (-1, -4)):
        moved, _ = _run(ctx, layer, (80, 132), (0, 0, 97, 41), (0, 0, 132, 80), (12 + dx, 12 + dy), 1, 3, 2, (200, 100, 50, 220))
        assert np.array_equal(moved, np.roll(base, (dy, dx), (0, 1))), (dx, dy)          # padded by more than the reach plus the move


# ---- symmetry ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s,r,p", [(2, 0, 0), (1, 3, 3), (0, 16, 2)])
def test_transposed_window_gives_the_transposed_image(ctx, layers, s, r, p):
    layer = layers["small"]
    t = np.ascontiguousarray(layer.transpose(1, 0, 2))
    a, want = _run(ctx, layer, (70, 132), (3, 2, 90, 37), (1, 2, 120, 66), (9, 14), s, r, p, (10, 200, 30, 180))
    b, _ = _run(ctx, t, (132, 70), (2, 3, 37, 90), (2, 1, 66, 120), (14, 9), s, r, p, (10, 200, 30, 180))
    assert np.array_equal(a, want)
    assert np.array_equal(a[2:68, 1:121].transpose(1, 0, 2), b[1:121, 2:68])


# ---- the tint over its domain ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("srgb", [False, True], ids=["unorm", "srgb"])
def test_tint_over_its_domain(ctx, srgb):
    """a 256 x 4 window whose alpha is the column, no stages: 256 calls with A = 0 .. 255 cover every (alpha, A), 86 calls at
    A = 255 whose colour bytes sweep 0 .. 255 cover every (C, a); each call has its own four rows of one destination"""
    layer = np.zeros((4, 256, 4), np.uint8)
    layer[..., 3] = np.arange(256)[None, :]
    layer[..., :3] = 77
    colours = [((3 * A) % 256, (255 - A) % 256, (A * 7 + 1) % 256, A) for A in range(256)]
    colours += [(k, (k + 86) % 256, (k + 172) % 256, 255) for k in range(86)]
    d = _dev(layer, (4 * len(colours), 256))
    want = d.image.copy()
    for i, c in enumerate(colours):
        _shadow(ctx, d, (0, 0, 256, 4), (0, 4 * i, 256, 4), (0, 0), 0, 0, 0, c, srgb)
        want = sr.shadow(layer, want, (0, 0, 256, 4), (0, 4 * i, 256, 4), (0, 0), 0, 0, 0, c, srgb)
    got = d.result(ctx)
    assert np.array_equal(got, want), np.argwhere(got != want)[:4]
    seen = {int(v) for c in colours[256:] for v in c[:3]}
    assert seen == set(range(256))


# ---- end to end ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("srgb", [False, True], ids=["unorm", "srgb"])
def test_text_with_its_shadow_over_a_frame(ctx, srgb):
    """one real-font line rendered with FR_TEXT_OVER over (0, 0, 0, 0); its shadow (s = 1, r = 3, p = 3, offset (2, 3), a
    translucent colour) composited onto a noise frame with fr_layer_over, then the text over it == layer_ref.composite of the
    twin's shadow and the same layer, byte for byte"""
    import torch
    from font_renderer_amd.text import _line
    font = load_font("DejaVuSans.ttf", allow_hinted=True)
    gs, places, runs, w, h = _line(font, "Shadow fjord, quay!", 19)
    cols = tg.colours(len(places), 5, opaque=True)
    flags = fr.FR_TEXT_OVER | (fr.FR_TEXT_SRGB if srgb else 0)
    dgs = fr.DeviceGlyphSet(ctx, gs)
    try:
        layer = tg.render_rgba(ctx, dgs, places, cols, runs, [(0, 0, 0, 0)], np.zeros((h, w, 4), np.uint8), 1, True, flags)
    finally:
        dgs.close()
    assert layer[..., 3].max() == 255 and (layer[..., 3] == 0).any()
    R, tx, ty = 10, 14, 12
    H, W = h + 2 * R + 8, (w + 2 * R + 8 + 3) // 4 * 4
    frame = tg.noise((H, W), 9)
    colour = (20, 30, 60, 170)
    dev_layer = torch.from_numpy(layer).to("cuda:0")
    dev_shadow = torch.full((H, W, 4), SENT, dtype=torch.uint8, device="cuda:0")
    dev_frame = torch.from_numpy(frame.copy()).to("cuda:0")
    torch.cuda.synchronize()
    fr.layer_shadow(ctx, dev_layer.data_ptr(), w, h, dev_shadow.data_ptr(), W, H, (0, 0, w, h), (0, 0, W, H), (tx + 2, ty + 3), 1, 3, 3, colour, srgb)
    fr.layer_over(ctx, dev_shadow.data_ptr(), W, H, dev_frame.data_ptr(), W, H, fr.make_blits([(0, 0, W, H, 0, 0, 255)]), srgb)
    fr.layer_over(ctx, dev_layer.data_ptr(), w, h, dev_frame.data_ptr(), W, H, fr.make_blits([(0, 0, w, h, tx, ty, 255)]), srgb)
    ctx.sync()
    shadow = sr.shadow_rect(layer, (0, 0, w, h), (W, H), (tx + 2, ty + 3), 1, 3, 3, colour, srgb)
    assert np.array_equal(dev_shadow.cpu().numpy(), shadow)
    want = lr.composite(layer, lr.composite(shadow, frame, [(0, 0, W, H, 0, 0, 255)], srgb), [(0, 0, w, h, tx, ty, 255)], srgb)
    got = dev_frame.cpu().numpy()
    assert np.array_equal(got, want), np.argwhere(got != want)[:4]
    assert not np.array_equal(got, frame) and 0 < shadow[..., 3].max() <= 170


def test_rgba_shadow_method(ctx, layers):
    layer = fr.RGBA(97, 41, layers["small"].reshape(-1, 4).copy())
    out = layer.shadow(offset=(2, 3), spread=1, blur_radius=2, blur_passes=2, rgba=(0, 0, 0, 128), pad=8, ctx=ctx)
    assert (out.width, out.height) == (113, 57)
    assert np.array_equal(out.as_3d(), sr.shadow_rect(layers["small"], (0, 0, 97, 41), (113, 57), (10, 11), 1, 2, 2, (0, 0, 0, 128)))


# ---- validation through the ABI --------------------------------------------------------------------------------------------
def test_refusals_leave_the_destination_untouched(ctx, layers):
    d = _dev(layers["small"], (50, 132))
    S, D = d.src, d.dst
    win, rect = (0, 0, 97, 41), (0, 0, 100, 50)

    def call(s=S, ss=97, srows=41, dp=D, ds=132, dr=50, window=win, rc=rect, stages=(1, 3, 3), flags=0):
        fr.layer_shadow(ctx, s, ss, srows, dp, ds, dr, window, rc, (0, 0), *stages, (1, 2, 3, 255), False, flags)

    cases = {
        "src NULL": (-1, "src", dict(s=0)),
        "dst NULL": (-1, "dst", dict(dp=0)),
        "shadow NULL": (-1, "shadow", dict(window=None)),
        "src not 4-byte aligned": (-1, "src", dict(s=S + 2, srows=40)),
        "dst not 4-byte aligned": (-1, "dst", dict(dp=D + 1, dr=49)),
        "src pitch beyond 2^26": (-1, "src", dict(ss=(1 << 26) + 1, srows=0)),
        "2^31 rows": (-4, "rows", dict(ds=0, dr=1 << 31, rc=(0, 0, 0, 0))),
        "window one pixel out": (-1, "window", dict(window=(1, 0, 97, 41))),
        "window one row out": (-1, "window", dict(window=(0, 1, 97, 41))),
        "rectangle one pixel out": (-1, "rectangle", dict(rc=(33, 0, 100, 50))),
        "rectangle one row out": (-1, "rectangle", dict(rc=(0, 1, 100, 50))),
        "spread 9": (-1, "spread", dict(stages=(9, 3, 3))),
        "radius 33": (-1, "blur_radius", dict(stages=(1, 33, 3))),
        "passes 4": (-1, "blur_passes", dict(stages=(1, 3, 4))),
        "unknown flag": (-1, "flag", dict(flags=2)),
        "a text flag": (-1, "flag", dict(flags=fr.FR_TEXT_OVER)),
        "the images alias": (-1, "overlap", dict(s=D, ss=132, srows=50)),
    }
    for what, (code, word, kw) in cases.items():
        with pytest.raises(fr.FrError) as e:
            call(**kw)
        assert e.value.code == code and word in str(e.value), (what, str(e.value))
    with pytest.raises(fr.FrError) as e:                               # NULL ctx
        L.check(L.load_library().fr_layer_shadow(None, S, 97, 41, D, 132, 50, None, 0))
    assert e.value.code == -1 and "ctx" in str(e.value)
    assert np.array_equal(d.result(ctx), d.image)
    call(stages=(8, 32, 3))                                            # the limits are valid
    assert np.array_equal(d.result(ctx), sr.shadow(layers["small"], d.image, win, rect, (0, 0), 8, 32, 3, (1, 2, 3, 255)))

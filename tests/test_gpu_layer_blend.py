"""fr_layer_blend on the GPU (include/fr_raster.h).  The expected image never comes from the code under test: it is the numpy
twin of the definition (tests/layer_blend_ref.py, itself held to the W3C formula in exact fractions and to the header's
consequences by tests/test_layer_blend_ref.py), or another device call where a consequence names one.  Destinations lie
between guard rows of sentinel bytes and whole arrays are compared, so a byte written outside a clipped rectangle fails; the
layer is compared with its copy afterwards."""
import numpy as np
import pytest

import font_renderer_amd as fr
import layer_blend_ref as br
import text_gpu as tg
from fixtures import load_font
from font_renderer_amd import _lib as L
from layer_gpu import SENT, Guarded, premultiplied

pytestmark = pytest.mark.gpu
SPACES = pytest.mark.parametrize("srgb", [False, True], ids=["unorm", "srgb"])
MODES = pytest.mark.parametrize("mode", range(br.MODES), ids=br.NAMES)
SOME_MODES = pytest.mark.parametrize("mode", [br.MULTIPLY, br.OVERLAY, br.DIFFERENCE, br.PLUS], ids=lambda m: br.NAMES[m])


def test_the_constants_are_the_twins():
    names = ("MULTIPLY", "SCREEN", "OVERLAY", "DARKEN", "LIGHTEN", "HARD_LIGHT", "DIFFERENCE", "EXCLUSION", "PLUS")
    assert [getattr(fr, "FR_BLEND_" + n) for n in names] == [getattr(br, n) for n in names] and fr.FR_BLEND_MODES == br.MODES == 9


def _run(ctx, layer, image, blits, mode, srgb=False, src_skip=0, dst_skip=0):
    """fr_layer_blend of `layer` into a guarded device copy of `image` -> the image after; the layer is checked against its copy"""
    d = Guarded(image, layer, dst_skip, src_skip)
    fr.layer_blend(ctx, d.src, layer.shape[1], layer.shape[0], d.dst, image.shape[1], image.shape[0], fr.make_blits(blits) if blits is not None else None, mode, srgb)
    return d.result(ctx)


def _check(ctx, layer, image, blits, mode, srgb=False, **skips):
    got = _run(ctx, layer, image, blits, mode, srgb, **skips)
    want = br.composite(layer, image, blits or [], mode, srgb)
    assert np.array_equal(got, want), (br.NAMES[mode], srgb, blits[:3] if blits else blits, skips, np.argwhere(got != want)[:4])
    return got


def _any_bytes(shape, seed):
    """arbitrary pixels, valid premultiplied or not"""
    return np.random.default_rng(seed).integers(0, 256, shape + (4,)).astype(np.uint8)


# ---- the arithmetic over its domain ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def domain():
    """blocks of 256 x 256, one above the other, the layer's index down the rows and the image's across the columns:
    (a) every (s_c, d_c) at the alpha pairs (255, 255), (255, 128), (128, 255) and (77, 200), the three colour bytes three
        different functions of the index (bytes above their alpha included);
    (b) every (s_a, d_a) at colours min(c, a), for three values of c turned through the channels;
    (c) every (s_c, o), the opacity down the rows, at two destinations"""
    v = np.arange(256)
    row, col = v[:, None] + 0 * v[None, :], v[None, :] + 0 * v[:, None]
    layers, images = [], []

    def block(sc, sa, dc, da):
        l, i = np.zeros((256, 256, 4), np.int64), np.zeros((256, 256, 4), np.int64)
        l[..., 0], l[..., 1], l[..., 2], l[..., 3] = sc[0], sc[1], sc[2], sa
        i[..., 0], i[..., 1], i[..., 2], i[..., 3] = dc[0], dc[1], dc[2], da
        layers.append(l.astype(np.uint8))
        images.append(i.astype(np.uint8))

    for p, q in ((255, 255), (255, 128), (128, 255), (77, 200)):
        block((row, (row + 85) % 256, 255 - row), p, (col, 255 - col, (col + 170) % 256), q)
    for c in ((255, 128, 40), (128, 40, 255), (40, 255, 128)):
        block([np.minimum(k, row) for k in c], row, [np.minimum(k, col) for k in c[::-1]], col)
    ab = (np.concatenate(layers), np.concatenate(images), [(0, 256 * k, 256, 256, 0, 256 * k, 255) for k in range(7)])
    # (c): the layer's colour across the columns, row y composited at opacity y
    layer = np.zeros((256, 256, 4), np.uint8)
    layer[..., 0], layer[..., 1], layer[..., 2], layer[..., 3] = col, (col + 85) % 256, 255 - col, np.where(row % 2 == 0, 255, col)
    image = np.zeros((512, 256, 4), np.uint8)
    image[:256], image[256:] = (10, 200, 90, 255), (60, 20, 0, 128)
    c = (layer, image, [(0, y, 256, 1, 0, y + 256 * half, y) for half in (0, 1) for y in range(256)])
    return ab, c


@SPACES
@MODES
def test_every_colour_pair_and_every_alpha_pair(ctx, domain, mode, srgb):
    (layer, image, blits), _ = domain
    got = _check(ctx, layer, image, blits, mode, srgb)
    assert not np.array_equal(got, image)


@SPACES
@MODES
def test_every_colour_at_every_opacity(ctx, domain, mode, srgb):
    _, (layer, image, blits) = domain
    got = _check(ctx, layer, image, blits, mode, srgb)
    assert np.array_equal(got[0], image[0]) and np.array_equal(got[256], image[256])      # o = 0: byte-identical


# ---- geometry ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene():
    """a 270 x 40 layer with runs of zero pixels beside inked ones, and images of arbitrary bytes in rows of 300 and 301"""
    rng = np.random.default_rng(31)
    layer = premultiplied(rng, (40, 270))
    layer[3:9, 8:40] = 0                                       # whole groups of four, on the 16-byte grid and off it
    layer[11:14, 101:131] = 0
    layer[:, 200:204] = 0
    layer[20, 60:64] = (255, 200, 255, 100)                    # not premultiplied
    return layer, {s: _any_bytes((45, s), s) for s in (300, 301)}


@SPACES
@SOME_MODES
@pytest.mark.parametrize("stride", [300, 301])
def test_a_blit_across_tile_borders_at_every_alignment(ctx, scene, stride, mode, srgb):
    """259 x 18: one tile border each way; dst_x 0, 1, 3 and src_x 0, 2 run the 16-byte path and the pixel path on either
    side (rows of 301 pixels leave the image's grid altogether); at opacity 255 and below"""
    layer, images = scene
    for dst_x in (0, 1, 3):
        for src_x in (0, 2):
            for o in (255, 140):
                _check(ctx, layer, images[stride], [(src_x, 1, 259, 18, dst_x, 2, o)], mode, srgb)
    _check(ctx, layer, images[stride], [(4, 0, 259, 18, 8, 0, 255)], mode, srgb, src_skip=1)          # the layer off the grid
    _check(ctx, layer, images[stride], [(4, 0, 259, 18, 8, 0, 255)], mode, srgb, dst_skip=3)          # the image off the grid


@SPACES
@SOME_MODES
def test_clipping_and_small_blits(ctx, scene, mode, srgb):
    layer, images = scene
    image = images[300]
    _check(ctx, layer, image, [(0, 0, 270, 40, -7, -5, 255)], mode, srgb)                   # negative dst_x and dst_y
    _check(ctx, layer, image, [(3, 2, 200, 30, 150, 30, 200)], mode, srgb)                  # clipped at the right and the bottom
    got = _check(ctx, layer, image, [(0, 0, 10, 10, 300, 0, 255), (0, 0, 10, 10, 5, -10, 255), (0, 0, 10, 10, 0, 45, 255)], mode, srgb)
    assert np.array_equal(got, image)                                                       # clipped away entirely
    _check(ctx, layer, image, [(21, 17, 1, 1, 299, 44, 255), (22, 17, 1, 1, 0, 0, 90), (60, 20, 1, 1, 150, 9, 255)], mode, srgb)   # 1 x 1
    # touching blits with different opacities, and one that does nothing
    _check(ctx, layer, image, [(0, 0, 20, 10, 10, 10, 255), (20, 0, 20, 10, 30, 10, 77), (0, 10, 40, 5, 10, 20, 1), (0, 15, 40, 5, 10, 25, 0)], mode, srgb)
    assert np.array_equal(_check(ctx, layer, image, [], mode, srgb), image)                 # n_blits = 0
    assert np.array_equal(_check(ctx, layer, image, None, mode, srgb), image)               # and no table at all


@SPACES
@MODES
def test_zero_groups_leave_their_destination_bit_identical(ctx, scene, mode, srgb):
    """groups of four zero layer pixels beside inked ones: the bytes under them, whatever they are, stay; the inked ones change"""
    layer, images = scene
    for stride, dst_x in ((300, 0), (300, 2), (301, 0)):
        image = images[stride]
        got = _check(ctx, layer, image, [(0, 0, 270, 40, dst_x, 3, 255)], mode, srgb)
        zero = ~layer.any(-1)
        under = got[3:43, dst_x:dst_x + 270]
        assert zero[3:9, 8:40].all() and np.array_equal(under[zero], image[3:43, dst_x:dst_x + 270][zero])
        assert not np.array_equal(under[~zero], image[3:43, dst_x:dst_x + 270][~zero])


# ---- the consequences, against device calls ------------------------------------------------------------------------------------
def _device(ctx, image, call, other):
    """call(dst, device address of other) on a guarded copy of image -> the image after"""
    import torch
    d = Guarded(image)
    dev = torch.from_numpy(np.ascontiguousarray(other)).to("cuda:0")
    torch.cuda.synchronize()
    call(d.dst, dev.data_ptr())
    return d.result(ctx)


@pytest.fixture(scope="module")
def two():
    """two images of one size, arbitrary bytes, with every corner byte present"""
    a, b = _any_bytes((37, 264), 41), _any_bytes((37, 264), 42)
    a[0, :6], b[0, :6] = ((0, 0, 0, 0), (255, 255, 255, 255), (255, 255, 255, 0), (0, 0, 0, 255), (128, 127, 1, 254), (1, 2, 3, 4)), (255, 0, 128, 127)
    return a, b


@pytest.fixture(scope="module")
def over_cleared(ctx, two):
    """fr_layer_over of the first image over a cleared one, on the device, per space and opacity"""
    a, _ = two
    clear = np.zeros_like(a)
    return {(srgb, o): _device(ctx, clear, lambda d, s: fr.layer_over(ctx, s, 264, 37, d, 264, 37, fr.make_blits([(0, 0, 264, 37, 0, 0, o)]), srgb), a)
            for srgb in (False, True) for o in (255, 99)}


@SPACES
@MODES
def test_consequence_3_over_a_cleared_image_every_mode_is_fr_layer_over(ctx, two, over_cleared, mode, srgb):
    a, _ = two
    for o in (255, 99):
        got = _run(ctx, a, np.zeros_like(a), [(0, 0, 264, 37, 0, 0, o)], mode, srgb)
        assert np.array_equal(got, over_cleared[srgb, o]), (o, np.argwhere(got != over_cleared[srgb, o])[:4])


@SPACES
@pytest.mark.parametrize("mode", br.SYMMETRIC, ids=[br.NAMES[m] for m in br.SYMMETRIC])
def test_consequence_4_symmetric_modes(ctx, two, mode, srgb):
    a, b = two
    whole = [(0, 0, 264, 37, 0, 0, 255)]
    ab, ba = _run(ctx, a, b, whole, mode, srgb), _run(ctx, b, a, whole, mode, srgb)
    assert np.array_equal(ab, ba) and not np.array_equal(ab, b)


@SPACES
def test_consequence_5_hard_light_is_overlay_swapped(ctx, two, srgb):
    a, b = two
    whole = [(0, 0, 264, 37, 0, 0, 255)]
    hard = _run(ctx, a, b, whole, br.HARD_LIGHT, srgb)
    assert np.array_equal(hard, _run(ctx, b, a, whole, br.OVERLAY, srgb))
    assert not np.array_equal(hard, _run(ctx, a, b, whole, br.OVERLAY, srgb))


# ---- end to end: a real font, one stream, no sync between render and blend ---------------------------------------------------
@SPACES
@pytest.mark.parametrize("mode", [br.MULTIPLY, br.DIFFERENCE], ids=["multiply", "difference"])
def test_a_text_line_blended_into_a_noise_frame(ctx, mode, srgb):
    """a DejaVuSans line rendered with FR_TEXT_OVER as a premultiplied layer and blended into a noise frame straight behind
    the render; the twin works on the layer as read back afterwards"""
    import torch
    from font_renderer_amd.text import _line
    font = load_font("DejaVuSans.ttf", allow_hinted=True)
    gs, places, runs, w, h = _line(font, "Highlight fjord, quay!", 19)
    cols = tg.colours(len(places), 5, opaque=False)
    pad = 5
    W, H = (w + 2 * pad + 3) // 4 * 4, h + 2 * pad
    frame = tg.noise((H, W), 9)
    text = torch.zeros((h, w, 4), dtype=torch.uint8, device="cuda:0")
    dst = torch.from_numpy(frame.copy()).to("cuda:0")
    torch.cuda.synchronize()
    dgs = fr.DeviceGlyphSet(ctx, gs)
    plan = fr.TextPlanRGBA(dgs, places, cols, runs, [(0, 0, 0, 0)], 1, fr.FR_SAMPLE_CENTER, fr.FR_TEXT_OVER | (fr.FR_TEXT_SRGB if srgb else 0))
    blits = [(0, 0, w, h, pad, pad, 230)]
    try:
        plan.render(text.data_ptr(), w, h)
        fr.layer_blend(ctx, text.data_ptr(), w, h, dst.data_ptr(), W, H, fr.make_blits(blits), mode, srgb)
        ctx.sync()
    finally:
        plan.close()
        dgs.close()
    layer, got = text.cpu().numpy(), dst.cpu().numpy()
    assert layer[..., 3].max() == 255 and (layer[..., 3] == 0).any() and ((layer[..., 3] > 0) & (layer[..., 3] < 255)).any()
    want = br.composite(layer, frame, blits, mode, srgb)
    assert np.array_equal(got, want), np.argwhere(got != want)[:4]
    assert not np.array_equal(got, frame) and np.array_equal(got[:pad], frame[:pad])


# ---- the interface ---------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_image_untouched(ctx, scene):
    """every refusal of the header through the C ABI: its code, and not a byte of the image or the layer changed"""
    import torch
    layer = scene[0]
    image = np.full((50, 132, 4), SENT, np.uint8)
    src, dst = (torch.from_numpy(a.copy()).to("cuda:0") for a in (layer, image))
    torch.cuda.synchronize()
    S, D = src.data_ptr(), dst.data_ptr()
    ok = [(0, 0, 10, 10, 0, 0, 255)]

    def call(s=S, ss=270, sr=40, d=D, ds=132, dr=50, rows=ok, mode=br.MULTIPLY, **kw):
        fr.layer_blend(ctx, s, ss, sr, d, ds, dr, fr.make_blits(rows), mode, **kw)

    cases = {
        "mode 9": (-1, dict(mode=9)),
        "mode 2^32 - 1": (-1, dict(mode=2 ** 32 - 1)),
        "opacity 256": (-1, dict(rows=[(0, 0, 10, 10, 0, 0, 256)])),
        "a blit one pixel out of the layer": (-1, dict(rows=[(261, 0, 10, 10, 0, 0, 255)])),
        "a blit one row out of the layer": (-1, dict(rows=[(0, 31, 10, 10, 0, 0, 255)])),
        "blits overlap by one pixel": (-1, dict(rows=[(0, 0, 20, 10, 10, 10, 255), (20, 0, 20, 10, 29, 19, 255)])),
        "the image is the layer": (-1, dict(s=D, ss=132, sr=50)),
        "the image ends in the layer": (-1, dict(s=D + 4 * 132 * 50 - 4, ss=1, sr=1, rows=[(0, 0, 1, 1, 0, 0, 255)])),
        "src not 4-byte aligned": (-1, dict(s=S + 2, sr=39)),
        "dst not 4-byte aligned": (-1, dict(d=D + 1, dr=49)),
        "src NULL": (-1, dict(s=0)),
        "dst NULL": (-1, dict(d=0)),
        "dst pitch beyond 2^26": (-1, dict(ds=(1 << 26) + 1, dr=0)),
        "src pitch beyond 2^26": (-1, dict(ss=(1 << 26) + 1, sr=0)),
        "2^31 rows of image": (-4, dict(ds=0, dr=1 << 31)),
        "2^31 rows of layer": (-4, dict(ss=0, sr=1 << 31)),
    }
    for what, (code, kw) in cases.items():
        with pytest.raises(fr.FrError) as e:
            call(**kw)
        assert e.value.code == code, (what, str(e.value))
    for flags in (fr.FR_LCD_BGR, fr.FR_MASK_PLANE, fr.FR_MASK_ERASE, 16, fr.FR_TEXT_OVER, 1 << 31):       # each foreign flag bit
        for srgb in (False, True):
            with pytest.raises(fr.FrError) as e:
                call(flags=flags, srgb=srgb)
            assert e.value.code == -1 and "flag" in str(e.value), flags
    with pytest.raises(fr.FrError) as e:                               # the flag bits are checked before the mode
        call(flags=fr.FR_LCD_BGR, mode=9)
    assert "flag" in str(e.value)
    with pytest.raises(fr.FrError) as e:                               # and the mode before the images
        call(s=0, mode=9)
    assert "mode" in str(e.value)
    lib = L.load_library()
    with pytest.raises(fr.FrError) as e:                               # NULL blits with a count
        L.check(lib.fr_layer_blend(ctx._h, S, 270, 40, D, 132, 50, None, 1, 0, 0))
    assert e.value.code == -1
    with pytest.raises(fr.FrError) as e:                               # NULL ctx
        L.check(lib.fr_layer_blend(None, S, 270, 40, D, 132, 50, None, 0, 0, 0))
    assert e.value.code == -1
    # valid calls that change nothing: no blits, 0 x anything, opacity 0, wholly clipped away
    fr.layer_blend(ctx, S, 270, 40, D, 132, 50, None, br.PLUS)
    call(rows=[(500, 500, 0, 3, 0, 0, 255)])
    call(rows=[(0, 0, 10, 10, 0, 0, 0)], mode=br.PLUS)
    call(rows=[(0, 0, 10, 10, 132, 0, 255)])
    ctx.sync()
    assert np.array_equal(dst.cpu().numpy(), image) and np.array_equal(src.cpu().numpy(), layer)
    # and the valid call draws
    call(rows=[(0, 0, 270, 40, 3, 3, 255)], mode=br.EXCLUSION)
    ctx.sync()
    assert np.array_equal(dst.cpu().numpy(), br.composite(layer, image, [(0, 0, 270, 40, 3, 3, 255)], br.EXCLUSION))


def test_rgba_blend_method(ctx, scene):
    layer = fr.RGBA(270, 40, scene[0].reshape(-1, 4).copy())
    start = premultiplied(np.random.default_rng(5), (45, 120))
    for mode, kw, row in ((br.SCREEN, dict(x=-4, y=9, opacity=77, srgb=True), (0, 0, 270, 40, -4, 9, 77)),
                          (br.HARD_LIGHT, dict(), (0, 0, 270, 40, 0, 0, 255)), (br.PLUS, dict(x=100, y=30), (0, 0, 270, 40, 100, 30, 255))):
        frame = fr.RGBA(120, 45, start.reshape(-1, 4).copy())
        assert frame.blend(layer, mode, ctx=ctx, **kw) is frame
        assert np.array_equal(frame.data.reshape(45, 120, 4), br.composite(scene[0], start, [row], mode, kw.get("srgb", False)))
    for bad in (dict(mode=9), dict(mode=-1), dict(mode=0, opacity=256)):
        with pytest.raises(ValueError):
            fr.RGBA(120, 45, start.reshape(-1, 4).copy()).blend(layer, ctx=ctx, **bad)

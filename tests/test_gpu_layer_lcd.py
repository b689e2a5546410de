"""fr_layer_lcd on the GPU (include/fr_raster.h).  The expected image never comes from the code under test: it is the numpy
twin of the definition (tests/layer_lcd_ref.py, itself held to a brute force and to the header's consequences by
tests/test_layer_lcd_ref.py), or a route through fr_layer_paint.  Destinations sit between guard rows, the plane is compared
with its copy after every call, and whole arrays are compared, so a byte written outside the clipped rectangles fails."""
import ctypes as C
from contextlib import closing

import numpy as np
import pytest

import font_renderer_amd as fr
import layer_lcd_ref as ll
import layer_paint_ref as pr
import layer_ref as lr
import text_twin as tw
from fixtures import load_font
from font_renderer_amd import _lib as L
from font_renderer_amd import text as T
from layer_gpu import Guarded, premultiplied

pytestmark = pytest.mark.gpu

FILTERS = {"default": None, "identity": ll.IDENTITY, "asymmetric": (0, 16, 64, 176, 0), "one_sided": (256, 0, 0, 0, 0)}
INVALID, UNSUPPORTED = -1, -4


class Plane:
    """a device copy of `plane` (rows, stride) u8, `skip` bytes off the allocation's start, between bytes of 255"""

    def __init__(self, plane, skip=0):
        import torch
        self.host, self.skip = np.ascontiguousarray(plane, np.uint8), skip
        flat = np.concatenate([np.full(skip, 255, np.uint8), self.host.reshape(-1), np.full(16, 255, np.uint8)])
        self._t = torch.from_numpy(flat).to("cuda:0")
        self.ptr = self._t.data_ptr() + skip
        self.rows, self.stride = self.host.shape

    def unchanged(self):
        got = self._t.cpu().numpy()
        return np.array_equal(got[self.skip:self.skip + self.host.size].reshape(self.host.shape), self.host) and (got[:self.skip] == 255).all() and (got[-16:] == 255).all()


def _run(ctx, plane, image, blits, weights=None, flags=0, skip=0, dst_skip=0):
    """fr_layer_lcd over guarded device copies -> the image after"""
    p, d = Plane(plane, skip), Guarded(image, dst_skip=dst_skip)
    fr.layer_lcd(ctx, p.ptr, p.stride, p.rows, d.dst, image.shape[1], image.shape[0], fr.make_lcd_blits(blits) if blits is not None else None, weights,
                 flags=flags)
    got = d.result(ctx)
    assert p.unchanged(), "the plane was written"
    return got


def _check(ctx, plane, image, blits, weights=None, flags=0, skip=0, dst_skip=0, changed=True):
    got = _run(ctx, plane, image, blits, weights, flags, skip, dst_skip)
    want = ll.lcd(plane, image, blits or [], weights, flags)
    assert np.array_equal(got, want), np.argwhere(got != want)[:4]
    if changed is not None:
        assert np.array_equal(got, image) != changed
    return got


def _textlike(rng, rows, stride):
    """runs of 0 and of 255 with values between: empty groups, opaque groups and edges"""
    v = rng.integers(0, 256, (rows, stride))
    kind = np.repeat(rng.integers(0, 3, (rows, (stride + 4) // 5)), 5, axis=1)[:, :stride]
    return np.where(kind == 0, 0, np.where(kind == 1, 255, v)).astype(np.uint8)


@pytest.fixture(scope="module")
def noise():
    rng = np.random.default_rng(77)
    return {shape: premultiplied(rng, shape) for shape in ((4, 16), (4, 260), (20, 8), (40, 300), (40, 301), (256, 256))}


# ---- impulses: every tap of every filter across every border of the ownership ------------------------------------------------

def _impulses(ctx, image, positions, name, flags, row=0):
    rows, stride = image.shape[:2]
    drawn = 0
    for q in positions:
        plane = np.zeros((rows, 3 * stride), np.uint8)
        plane[row, q] = 255
        # (a one-sided filter moves an impulse at the window's end out of it: nothing is drawn then, as the twin says)
        got = _check(ctx, plane, image, [(0, 0, stride, rows, 0, 0, (255, 180, 40, 255))], FILTERS[name], flags, changed=None)
        other = np.delete(got, row, axis=0)
        assert np.array_equal(other, np.delete(image, row, axis=0)), "an impulse reached another row"
        drawn += not np.array_equal(got, image)
    assert drawn >= len(positions) - 2


@pytest.mark.parametrize("flags", [0, ll.SRGB], ids=["unorm", "srgb"])
@pytest.mark.parametrize("name", sorted(FILTERS))
def test_impulse_at_every_sub_pixel_of_a_group_and_across_a_lane_border(ctx, noise, name, flags):
    """16 x 4 pixels: lane 1's twelve sub-pixels are elements 12 .. 23; pixels 3 | 4 meet at elements 11 | 12; the window's
    two ends are in (elements 0, 1 and 46, 47)"""
    _impulses(ctx, noise[(4, 16)], range(48), name, flags, row=1)


@pytest.mark.parametrize("name", sorted(FILTERS))
def test_impulse_across_a_tile_border(ctx, noise, name):
    """260 pixels: lane 63 of the first tile and lane 0 of the second, whose side taps are fetched, meet at pixels 255 | 256"""
    _impulses(ctx, noise[(4, 260)], range(3 * 255 - 3, 3 * 256 + 6), name, ll.SRGB if name == "asymmetric" else 0, row=2)


@pytest.mark.parametrize("name", sorted(FILTERS))
def test_impulse_across_a_tile_row_border(ctx, noise, name):
    for row in (15, 16):
        _impulses(ctx, noise[(20, 8)], (0, 7, 13, 23), name, 0, row=row)


# ---- the window's edges and the two access paths -----------------------------------------------------------------------------

@pytest.mark.parametrize("flags", [0, 3], ids=["unorm", "srgb_bgr"])
@pytest.mark.parametrize("name", ["default", "one_sided", "asymmetric"])
def test_neighbours_of_the_window_count_as_zero(ctx, noise, name, flags):
    """255 on all four sides of the window: the twin sees zeros there"""
    rng = np.random.default_rng(5)
    image = noise[(40, 300)]
    # the rectangle starts one pixel right of the lane grid: dwords from three elements left of the window, masked; dwords; bytes; bytes
    for sx, stride in ((3, 880), (7, 880), (5, 879), (4, 878)):
        plane = np.full((39, stride), 255, np.uint8)
        plane[2:37, sx:sx + 3 * 290] = _textlike(rng, 35, 3 * 290)
        _check(ctx, plane, image, [(sx, 2, 290, 35, 5, 3, (20, 200, 255, 230))], FILTERS[name], flags)


@pytest.mark.parametrize("extra", [0, 1, 2, 3, 4, 5])
def test_every_pitch_and_every_start(ctx, noise, extra):
    """w = 44: rows of 132 + extra bytes with src_x in 0 .. 3: refused where the window does not fit; where src_x = extra it
    ends at the last byte of the plane's last row.  Pitches 132 and 136 allow dwords, the others take bytes; the two
    destinations start on and off the lane grid, which moves a lane's first element by three per pixel."""
    rng = np.random.default_rng(extra)
    image = noise[(40, 300)]
    stride = 132 + extra
    for sx in range(4):
        plane = _textlike(rng, 19, stride)
        p, d = Plane(plane), Guarded(image)
        blits = [(sx, 2, 44, 17, 8 + sx, 1, (255, 255, 255, 255))]
        if sx > extra:
            rc = ctx._lib.fr_layer_lcd(ctx._h, C.c_void_p(p.ptr), stride, 19, C.c_void_p(d.dst), 300, 40, L.ptr(fr.make_lcd_blits(blits)), 1, None, 0)
            assert rc == INVALID
            assert np.array_equal(d.result(ctx), image)
            continue
        _check(ctx, plane, image, blits)
        _check(ctx, plane, image, [(sx, 2, 44, 17, 8, 1, (9, 80, 255, 200))], FILTERS["asymmetric"], ll.SRGB)


@pytest.mark.parametrize("skip", [1, 2, 3])
def test_plane_off_the_allocation_by_bytes(ctx, noise, skip):
    rng = np.random.default_rng(skip)
    plane = _textlike(rng, 20, 400)
    for sx in (0, 4 - skip, 1):                                 # bytes; dwords (cov + src_x on the grid); bytes
        _check(ctx, plane, noise[(40, 300)], [(sx, 1, 130, 19, 12, 2, (255, 255, 255, 255))], None, 0, skip=skip)
    _check(ctx, plane, noise[(40, 301)], [(4 - skip, 0, 130, 20, 1, 0, (0, 0, 0, 255))], None, ll.SRGB, skip=skip, dst_skip=1)


@pytest.mark.parametrize("flags", [0, 1, 2, 3])
def test_two_tiles_across_three_down_ragged(ctx, noise, flags):
    """300 x 40 with a margin: rows of 300 on the 16-byte grid and rows of 301 one pixel off it"""
    rng = np.random.default_rng(9)
    plane = _textlike(rng, 40, 912)
    _check(ctx, plane, noise[(40, 300)], [(7, 2, 290, 35, 5, 3, (200, 30, 90, 255))], None, flags)
    _check(ctx, plane, noise[(40, 301)], [(9, 2, 290, 35, 5, 3, (200, 30, 90, 140))], None, flags, dst_skip=1)


# ---- clipping ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("flags", [0, 1], ids=["unorm", "srgb"])
def test_clipping(ctx, noise, flags):
    rng = np.random.default_rng(10)
    plane, image = _textlike(rng, 40, 912), noise[(40, 300)]
    white = (255, 255, 255, 255)
    _check(ctx, plane, image, [(0, 0, 300, 40, -7, -5, white)], None, flags)                    # taps left of column 0 are in the window
    _check(ctx, plane, image, [(0, 0, 300, 40, 200, 30, white)], None, flags)                   # over the right and bottom edges
    _check(ctx, plane, image, [(0, 0, 300, 40, 300, 0, white)], None, flags, changed=False)     # clipped away
    _check(ctx, plane, image, [(0, 0, 300, 40, 0, -40, white)], None, flags, changed=False)
    _check(ctx, plane, image, [(0, 0, 0, 40, 0, 0, white)], None, flags, changed=False)         # w = 0
    _check(ctx, plane, image, [(5000, 5000, 10, 0, 0, 0, white)], None, flags, changed=False)   # h = 0, the window anywhere
    _check(ctx, plane, image, [], None, flags, changed=False)
    _check(ctx, plane, image, None, None, flags, changed=False)
    # two blits of different colours in one tile, touching
    _check(ctx, plane, image, [(0, 0, 50, 12, 10, 2, (255, 0, 0, 255)), (300, 5, 61, 12, 60, 2, (0, 90, 255, 128))], None, flags)


def test_300_one_pixel_blits(ctx, noise):
    rng = np.random.default_rng(11)
    plane, image = _textlike(rng, 40, 912), noise[(40, 300)]
    plane[plane == 0] = 9                                       # every blit draws
    at = rng.permutation(300 * 40)[:300]
    blits = [(int(rng.integers(0, 909)), int(rng.integers(0, 40)), 1, 1, int(k % 300), int(k // 300), tuple(int(v) for v in rng.integers(1, 256, 4))) for k in at]
    _check(ctx, plane, image, blits, None, 0)
    _check(ctx, plane, image, blits, FILTERS["identity"], 3)


# ---- arithmetic, on the device -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("flags", [0, 1], ids=["unorm", "srgb"])
@pytest.mark.parametrize("A", [0, 1, 127, 128, 254, 255])
def test_every_f_and_A(ctx, noise, A, flags):
    """f = X in column X through the identity filter"""
    plane = np.repeat(np.arange(256, dtype=np.uint8), 3)[None, :].repeat(256, axis=0)
    _check(ctx, plane, noise[(256, 256)], [(0, 0, 256, 256, 0, 0, (250, 128, 3, A))], ll.IDENTITY, flags, changed=A != 0)


@pytest.mark.parametrize("flags", [0, 1], ids=["unorm", "srgb"])
@pytest.mark.parametrize("a", [1, 64, 128, 254, 255])
def test_every_colour_and_destination_byte(ctx, a, flags):
    """row C is a blit of colour (C, C, C, 255), column d holds (d, 255 - d, d, 255): every (C, d) pair at a_b = a"""
    image = np.zeros((256, 256, 4), np.uint8)
    image[..., 0] = image[..., 2] = np.arange(256)[None, :]
    image[..., 1] = 255 - np.arange(256)[None, :]
    image[..., 3] = 255
    plane = np.full((256, 768), a, np.uint8)
    blits = [(0, c, 256, 1, 0, c, (c, c, c, 255)) for c in range(256)]
    _check(ctx, plane, image, blits, ll.IDENTITY, flags)


@pytest.mark.parametrize("flags", [0, 1, 2, 3])
def test_three_alphas_per_pixel(ctx, flags):
    """independent sub-pixels through the identity filter over destination alphas 0, 100 and 255: the alpha rule, and with
    flags = 0 a premultiplied image stays premultiplied (consequence 6)"""
    rng = np.random.default_rng(12)
    plane = rng.integers(0, 256, (48, 900)).astype(np.uint8)
    plane[:, 300:400] = rng.choice(np.array([0, 255], np.uint8), (48, 100))     # channels at 0 and at 255 in one pixel
    image = np.zeros((48, 300, 4), np.uint8)
    image[..., 3] = np.repeat(np.array([0, 100, 255], np.uint8), 100)[None, :]
    image[..., :3] = rng.integers(0, 256, (48, 300, 3)) * image[..., 3:].astype(np.int64) // 255
    for colour in ((255, 255, 255, 255), (250, 3, 128, 200)):
        got = _check(ctx, plane, image, [(0, 0, 300, 48, 0, 0, colour)], ll.IDENTITY, flags)
        if flags == 0:
            assert (got[..., :3] <= got[..., 3:]).all()
        assert (got[:, 200:, 3] == 255).all()                   # consequence 2


# ---- flags -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("srgb", [0, 1])
def test_bgr_is_the_byte_swapped_call(ctx, noise, srgb):
    rng = np.random.default_rng(13)
    plane, image = _textlike(rng, 40, 912), noise[(40, 300)]
    swap = lambda im: np.ascontiguousarray(im[..., [2, 1, 0, 3]])
    got = _run(ctx, plane, image, [(3, 0, 300, 40, 0, 0, (200, 30, 90, 180))], None, srgb | ll.BGR)
    want = swap(_run(ctx, plane, swap(image), [(3, 0, 300, 40, 0, 0, (90, 30, 200, 180))], None, srgb))
    assert np.array_equal(got, want) and not np.array_equal(got, image)


def test_the_other_layer_calls_refuse_flag_2(ctx, noise):
    image = noise[(40, 300)]
    d = Guarded(image, premultiplied(np.random.default_rng(1), (40, 300)))
    calls = [lambda: fr.layer_over(ctx, d.src, 300, 40, d.dst, 300, 40, fr.make_blits([(0, 0, 10, 10, 0, 0, 255)]), flags=L.FR_LCD_BGR),
             lambda: fr.layer_rects(ctx, d.dst, 300, 40, fr.make_rects([(0, 0, 640, 640, (1, 2, 3, 255))]), flags=L.FR_LCD_BGR),
             lambda: fr.layer_paint(ctx, d.src, 300, 40, d.dst, 300, 40, fr.make_gradient_linear(0, 0, 640, 0, [(0, (1, 2, 3, 255))]), (0, 0, 10, 10), flags=L.FR_LCD_BGR),
             lambda: fr.layer_shadow(ctx, d.src, 300, 40, d.dst, 300, 40, (0, 0, 10, 10), (0, 0, 10, 10), flags=L.FR_LCD_BGR)]
    for call in calls:
        with pytest.raises(fr.FrError) as e:
            call()
        assert e.value.code == INVALID and "flag" in str(e.value)
    assert np.array_equal(d.result(ctx), image)


# ---- routes --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("flags", [0, 1, 2, 3])
def test_identity_filter_equals_a_one_stop_paint_on_the_device(ctx, noise, flags):
    """consequence 5 against fr_layer_paint itself"""
    rng = np.random.default_rng(14)
    k = _textlike(rng, 35, 290)
    layer = np.zeros((35, 290, 4), np.uint8)
    layer[..., 3] = k
    image, colour = noise[(40, 300)], (200, 30, 90, 180)
    got = _check(ctx, np.repeat(k, 3, axis=1), image, [(0, 0, 290, 35, 5, 3, colour)], ll.IDENTITY, flags)
    d = Guarded(image, layer)
    fr.layer_paint(ctx, d.src, 290, 35, d.dst, 300, 40, fr.make_gradient_linear(0, 0, 640, 0, [(0, colour)]), (0, 0, 290, 35), (5, 3), bool(flags & 1))
    assert np.array_equal(got, d.result(ctx))


def _line(x):
    font = load_font("DejaVuSans.ttf", allow_hinted=True)
    return font, T.lcd_line(font, "Hamburgefont", 16, x, 17.0, 120, 24)


@pytest.fixture(scope="module")
def frame():
    return premultiplied(np.random.default_rng(15), (24, 120))


@pytest.mark.parametrize("srgb", [False, True], ids=["unorm", "srgb"])
@pytest.mark.parametrize("third", [0, 1, 2])
def test_real_font_line(ctx, frame, third, srgb):
    """draw_text_lcd with the pen at three thirds of a pixel: the image is the twin's of the plane the device made"""
    font = load_font("DejaVuSans.ttf", allow_hinted=True)
    im = fr.RGBA(120, 24, frame.reshape(-1, 4).copy())
    im, plane = fr.draw_text_lcd(im, font, "Hamburgefont", 16, 4 + third / 3, 17, (20, 10, 0, 255), srgb=srgb, return_plane=True, ctx=ctx)
    cov = plane.as_2d()
    assert cov.shape == (24, 360) and cov.max() == 255 and (cov == 0).mean() > 0.5
    want = ll.lcd(cov, frame, [(0, 0, 120, 24, 0, 0, (20, 10, 0, 255))], None, ll.SRGB if srgb else 0)
    assert np.array_equal(im.as_3d(), want) and not np.array_equal(want, frame)
    # sub-pixel text is coloured at its edges: some pixel's three channels moved by different amounts
    assert (np.ptp(want[..., :3].astype(int) - frame[..., :3].astype(int), axis=-1) > 0).any()


@pytest.mark.parametrize("third", [0, 1, 2])
def test_real_font_plane_is_the_affine_twin(ctx, third):
    font, (gs, places, runs) = _line(4 + third / 3)
    with closing(fr.DeviceGlyphSet(ctx, gs)) as dgs, closing(fr.TextPlan(dgs, places, runs, fr.FR_COVERAGE_U8, 4, fr.FR_SAMPLE_CENTER, fr.FR_FILL_CONSISTENT)) as plan:
        from font_renderer_amd.device import round_trip
        got = round_trip(ctx, lambda p: plan.render(p, 360, 24), (24 * 360,)).reshape(24, 360)
    want = tw.render_run("affine", gs, places, runs[0], n=4, center=True, fill=True)
    assert np.array_equal(got, want) and got.max() == 255


def test_stream_order_render_lcd_over(ctx, frame):
    """the plane's render, fr_layer_lcd and fr_layer_over on top, queued with no sync between them"""
    import torch
    font, (gs, places, runs) = _line(4.25)
    layer = premultiplied(np.random.default_rng(16), (24, 120))
    d = Guarded(frame, layer)
    cov = torch.empty(24 * 360, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    blits = fr.make_lcd_blits([(0, 0, 120, 24, 0, 0, (255, 255, 255, 255))])
    with closing(fr.DeviceGlyphSet(ctx, gs)) as dgs, closing(fr.TextPlan(dgs, places, runs, fr.FR_COVERAGE_U8, 4, fr.FR_SAMPLE_CENTER, fr.FR_FILL_CONSISTENT)) as plan:
        plan.render(cov.data_ptr(), 360, 24)
        fr.layer_lcd(ctx, cov.data_ptr(), 360, 24, d.dst, 120, 24, blits)
        fr.layer_over(ctx, d.src, 120, 24, d.dst, 120, 24, fr.make_blits([(0, 0, 120, 24, 0, 0, 200)]))
        got = d.result(ctx)
    plane = cov.cpu().numpy().reshape(24, 360)
    text = ll.lcd(plane, frame, [(0, 0, 120, 24, 0, 0, (255, 255, 255, 255))])
    assert plane.max() == 255 and not np.array_equal(text, frame)
    assert np.array_equal(got, lr.composite(layer, text, [(0, 0, 120, 24, 0, 0, 200)]))


def test_rgba_draw_lcd_and_render_text_lcd(ctx, frame):
    rng = np.random.default_rng(17)
    plane = _textlike(rng, 20, 90)
    im = fr.RGBA(120, 24, frame.reshape(-1, 4).copy()).draw_lcd(fr.Gray(90, 20, plane.reshape(-1)), 7, -3, (9, 8, 7, 200), weights=(0, 16, 64, 176, 0), srgb=True, bgr=True, ctx=ctx)
    assert np.array_equal(im.as_3d(), ll.lcd(plane, frame, [(0, 0, 30, 20, 7, -3, (9, 8, 7, 200))], (0, 16, 64, 176, 0), 3))
    out = fr.render_text_lcd(load_font("DejaVuSans.ttf", allow_hinted=True), "fi", 16, 2.5, 14, 30, 18, ctx=ctx)
    px = out.as_3d()
    assert (px[..., 3] == 255).all() and px.min() < 64 and (px[0] == 255).all()


# ---- validation ----------------------------------------------------------------------------------------------------------------

def test_every_refusal_leaves_the_image_untouched(ctx, noise):
    image = noise[(40, 300)]
    plane = np.full((40, 912), 200, np.uint8)
    p, d = Plane(plane), Guarded(image)
    one = fr.make_lcd_blits([(0, 0, 10, 10, 0, 0, (255, 255, 255, 255))])
    W = lambda *v: (C.c_uint16 * 5)(*v)

    def call(h=None, cov=p.ptr, cs=912, cr=40, dst=d.dst, ds=300, dr=40, blits=one, n=1, weights=None, flags=0):
        return ctx._lib.fr_layer_lcd(ctx._h if h is None else h, C.c_void_p(cov), cs, cr, C.c_void_p(dst), ds, dr, None if blits is None else L.ptr(blits), n, weights, flags)

    def blit(*row):
        return fr.make_lcd_blits([row + ((255, 255, 255, 255),)])

    two = fr.make_lcd_blits([(0, 0, 20, 10, 10, 10, (1, 2, 3, 255)), (60, 0, 20, 10, 29, 19, (1, 2, 3, 255))])
    assert call(h=C.c_void_p(None)) == INVALID
    assert call(flags=4) == INVALID and call(flags=L.FR_TEXT_SRGB | L.FR_TEXT_OVER) == INVALID
    assert call(cov=None) == INVALID
    assert call(cs=(1 << 26) + 1) == INVALID
    assert call(dst=None) == INVALID and call(dst=d.dst + 2) == INVALID
    assert call(ds=(1 << 26) + 1) == INVALID
    assert call(dr=1 << 31) == UNSUPPORTED and call(cr=1 << 31) == UNSUPPORTED
    assert call(blits=None) == INVALID
    assert call(weights=W(8, 77, 85, 77, 8)) == INVALID and call(weights=W(8, 77, 87, 77, 8)) == INVALID and call(weights=W(65535, 257, 0, 0, 0)) == INVALID
    assert call(blits=blit(883, 0, 10, 10, 0, 0)) == INVALID and call(blits=blit(0, 31, 10, 10, 0, 0)) == INVALID
    assert call(blits=blit(0xffffffff, 0, 2, 2, 0, 0)) == INVALID and call(blits=blit(0, 0, 0x55555556, 2, 0, 0)) == INVALID
    assert call(blits=two, n=2) == INVALID
    assert call(cov=d.dst, cs=1200, cr=40) == INVALID and call(cov=d.dst + 4 * 300 * 40 - 1, cs=16, cr=1, blits=blit(0, 0, 5, 1, 0, 0)) == INVALID
    # (refused before anything is launched: the addresses only have to be apart)
    big = blit(0, 0, 1 << 16, (1 << 18) + 1, 0, 0)
    assert call(cov=1 << 40, dst=1 << 44, cs=3 << 16, cr=(1 << 18) + 1, ds=1 << 16, dr=(1 << 18) + 1, blits=big) == UNSUPPORTED
    # the order: the earlier rule's code wins
    assert call(flags=4, dr=1 << 31) == INVALID and call(dst=d.dst + 2, dr=1 << 31) == INVALID and call(dr=1 << 31, blits=None) == UNSUPPORTED
    assert "weights" in _message(call(weights=W(1, 0, 0, 0, 0), blits=blit(883, 0, 10, 10, 0, 0)))
    assert "overlap in the destination" in _message(call(cov=d.dst, cs=1200, cr=40, blits=two, n=2))
    assert "overlap in memory" in _message(call(cov=1 << 44, dst=1 << 44, cs=3 << 16, cr=(1 << 18) + 1, ds=1 << 16, dr=(1 << 18) + 1, blits=big))
    assert np.array_equal(d.result(ctx), image) and p.unchanged()
    # and what is valid beside them
    assert call(n=0, blits=None) == 0 and call(blits=blit(882, 30, 10, 10, 0, 0), weights=W(0, 0, 0, 0, 256), flags=3) == 0
    got = d.result(ctx)
    want = ll.lcd(plane, image, [(882, 30, 10, 10, 0, 0, (255, 255, 255, 255))], (0, 0, 0, 0, 256), 3)
    assert np.array_equal(got, want) and p.unchanged()


def _message(rc):
    assert rc == INVALID
    return L.load_library().fr_last_error().decode()

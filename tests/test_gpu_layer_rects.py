"""fr_layer_rects on the GPU (include/fr_raster.h).  The expected image never comes from the code under test: it is the
numpy twin of the definition (tests/layer_rects_ref.py, itself held to exact fractions and to the header's consequences by
tests/test_layer_rects_ref.py), or the route through fr_layer_shadow and fr_layer_over.  Destinations are noise or
sentinel-filled with guard rows around them, and whole arrays are compared, so a byte written outside a bounding box
fails."""
import numpy as np
import pytest

import font_renderer_amd as fr
import layer_ref as lr
import layer_rects_ref as rr
from fixtures import load_font
from font_renderer_amd import _lib as L
from layer_gpu import SENT, Guarded, premultiplied

pytestmark = pytest.mark.gpu
MAXI, MINI = 2 ** 31 - 1, -2 ** 31


def _rects(ctx, image, rows, srgb=False, dst_skip=0):
    """fr_layer_rects of `rows` (edges in 1/64 pixel) over a guarded device copy of `image` (rows, stride, 4) -> the image
    after.  dst_skip: pixels the device array is moved by, to leave the 16-byte grid."""
    d = Guarded(image, dst_skip=dst_skip)
    fr.layer_rects(ctx, d.dst, image.shape[1], image.shape[0], None if rows is None else fr.make_rects(rows), srgb)
    return d.result(ctx)


@pytest.fixture(scope="module")
def noise():
    return premultiplied(np.random.default_rng(31), (130, 130))


@pytest.mark.parametrize("srgb", [False, True], ids=["unorm", "srgb"])
@pytest.mark.parametrize("alpha", [255, 128, 1])
def test_every_coverage(ctx, noise, alpha, srgb):
    """65 x 65 rectangles in one call: rectangle (i, j) sits in pixel (2 i, 2 j) with width i / 64 and height j / 64, so
    every (cx, cy) occurs, over noise (every destination alpha among them)"""
    rows = [(128 * i, 128 * j, 128 * i + i, 128 * j + j, (200, 60, 250, alpha)) for j in range(65) for i in range(65)]
    assert len(rows) == 4225
    got = _rects(ctx, noise, rows, srgb)
    want = rr.rects(noise, rows, srgb)
    assert np.array_equal(got, want), np.argwhere(got != want)[:4]
    assert np.array_equal(got[1::2], noise[1::2]) and np.array_equal(got[:, 1::2], noise[:, 1::2])
    assert not np.array_equal(got, noise)


def _partial(a):
    """(cy, A) with cy < 64 whose row coverage k = (255 * 64 * cy + 2048) div 4096 gives m(k, A) = a, or None: the largest
    coverage of a partly covered pixel is 251, so 254 and 255 are only reached through rgba[3]"""
    for cy in range(1, 64):
        k = (255 * 64 * cy + 2048) // 4096
        for A in range(255, 0, -1):
            if int(lr.m(k, A)) == a:
                return cy, A
    return None


@pytest.mark.parametrize("srgb", [False, True], ids=["unorm", "srgb"])
@pytest.mark.parametrize("a", [1, 127, 128, 254, 255])
@pytest.mark.parametrize("route", ["alpha", "coverage"])
def test_every_colour_pair(ctx, a, route, srgb):
    """256 rectangles, one row tall and 256 wide, C = the row in all three channels, over d_c = the column: the whole
    (C, d_c) domain of D, E and m at source alpha a, reached through rgba[3] at full coverage or through a partly covered
    row"""
    if route == "alpha":
        cy, A = 64, a
    else:
        found = _partial(a)
        if found is None:
            assert a > max((255 * cx * cy + 2048) // 4096 for cx in range(65) for cy in range(64)) == 251      # m(k, A) <= k
            return
        cy, A = found
    image = np.zeros((256, 256, 4), np.uint8)
    image[..., :3] = np.arange(256)[None, :, None]
    image[..., 3] = 255
    rows = [(0, 64 * c, 256 * 64, 64 * c + cy, (c, c, c, A)) for c in range(256)]
    assert int(lr.m(rr.coverage(rows[3], 256, 256)[3, 100], A)) == a
    got = _rects(ctx, image, rows, srgb)
    want = rr.rects(image, rows, srgb)
    assert np.array_equal(got, want), np.argwhere(got != want)[:4]
    assert not np.array_equal(got, image)


GEOMETRY = {
    "across_the_16_row_borders": [(64 * 3 + 9, 64 * 15 + 40, 64 * 90 + 3, 64 * 16 + 20, (250, 10, 60, 255)), (64 * 100, 64 * 10, 64 * 101 + 1, 64 * 40 + 63, (5, 200, 90, 140)),
                                  (64 * 20, 64 * 31, 64 * 60, 64 * 33, (90, 90, 255, 255))],
    "negative_and_far_outside_edges": [(-5000, -300, 64 * 40 + 7, 64 * 9 + 1, (10, 250, 30, 200)), (64 * 100 + 32, 64 * 30 + 32, 10 ** 9, 10 ** 9, (240, 240, 10, 255)),
                                       (-10 ** 9, 64 * 44, 10 ** 9, 64 * 45 + 32, (1, 2, 3, 99))],
    "edges_at_the_int32_limits": [(MINI, MINI, MAXI, 64 * 2 + 5, (70, 80, 90, 128)), (64 * 120 + 11, 64 * 5, MAXI, MAXI, (200, 100, 50, 255)),
                                  (MINI + 1, 64 * 47 + 1, 64 * 20 + 32, MAXI, (3, 3, 3, 255))],
    "clipped_away_entirely": [(64 * 132 + 63, 0, 64 * 140, 64 * 10, (9, 9, 9, 255)), (64 * 132, 0, 64 * 140, 64 * 10, (9, 9, 9, 255)), (0, 64 * 50, 64 * 10, 64 * 60, (9, 9, 9, 255)),
                              (-640, -640, 0, 0, (9, 9, 9, 255)), (MAXI - 64, MAXI - 64, MAXI, MAXI, (9, 9, 9, 255)), (MINI, MINI, MINI + 64, MINI + 64, (9, 9, 9, 255)),
                              (640, 640, 64, 64, (9, 9, 9, 255)), (64, 64, 640, 64, (9, 9, 9, 255))],
    "ragged_groups_and_single_pixels": [(64 * 5, 64, 64 * 6, 128, (255, 0, 0, 255)), (64 * 9 + 1, 64 * 3, 64 * 14 + 63, 64 * 4, (0, 255, 0, 255)),
                                        (64 * 17, 64 * 5, 64 * 23, 64 * 9, (0, 0, 255, 77)), (64 * 22, 64 * 7, 64 * 31, 64 * 8, (255, 255, 0, 255)),
                                        (64 * 126, 64 * 20, 64 * 131, 64 * 22, (1, 255, 255, 255)), (64 * 129 + 32, 64 * 48, 64 * 200, 64 * 70, (255, 1, 255, 31))],
}
WIDE = {
    "across_the_256_column_border": [(64 * 255 + 63, 64 * 2, 64 * 256 + 1, 64 * 3, (250, 10, 60, 255)), (64 * 250, 64 * 15 + 32, 64 * 262 + 5, 64 * 17, (5, 200, 90, 140)),
                                     (64 * 100, 64 * 5, 64 * 290, 64 * 6, (90, 90, 255, 255)), (64 * 256, 64 * 8, 64 * 260, 64 * 12, (7, 7, 7, 200))],
}


@pytest.mark.parametrize("srgb", [False, True], ids=["unorm", "srgb"])
@pytest.mark.parametrize("stride,dst_skip", [(131, 0), (132, 0), (132, 3)], ids=["rows131", "rows132", "dst_off_grid"])
@pytest.mark.parametrize("case", sorted(GEOMETRY))
def test_geometry(ctx, case, stride, dst_skip, srgb):
    """a sentinel-filled 130 x 50 destination in rows of `stride` pixels: rows of 131 and a destination off the 16-byte grid
    take the pixel-by-pixel path, rows of 132 the 16-byte path with ragged edges"""
    image = np.full((50, stride, 4), SENT, np.uint8)
    got = _rects(ctx, image, GEOMETRY[case], srgb, dst_skip)
    want = rr.rects(image, GEOMETRY[case], srgb)
    assert np.array_equal(got, want), (case, np.argwhere(got != want)[:4])
    assert np.array_equal(got, image) == (case == "clipped_away_entirely")


@pytest.mark.parametrize("srgb", [False, True], ids=["unorm", "srgb"])
@pytest.mark.parametrize("stride,dst_skip", [(291, 0), (292, 0), (292, 1)], ids=["rows291", "rows292", "dst_off_grid"])
@pytest.mark.parametrize("case", sorted(WIDE))
def test_geometry_across_tile_columns(ctx, case, stride, dst_skip, srgb):
    """the same over a 290 x 20 destination, which has a second column of tiles"""
    image = np.full((20, stride, 4), SENT, np.uint8)
    got = _rects(ctx, image, WIDE[case], srgb, dst_skip)
    want = rr.rects(image, WIDE[case], srgb)
    assert np.array_equal(got, want), (case, np.argwhere(got != want)[:4])


@pytest.mark.parametrize("srgb", [False, True], ids=["unorm", "srgb"])
def test_order(ctx, srgb):
    """three translucent rectangles that overlap: the list and the reversed list both equal the twin, and differ"""
    image = np.zeros((40, 132, 4), np.uint8)
    image[:] = (30, 60, 90, 200)
    rows = [(64 * 5, 64 * 5, 64 * 60 + 20, 64 * 30 + 7, (255, 0, 0, 128)), (64 * 30 + 11, 64 * 10, 64 * 100, 64 * 35, (0, 255, 0, 128)),
            (64 * 20, 64 * 18 + 3, 64 * 120, 64 * 25, (0, 0, 255, 200))]
    forward, backward = _rects(ctx, image, rows, srgb), _rects(ctx, image, rows[::-1], srgb)
    assert np.array_equal(forward, rr.rects(image, rows, srgb))
    assert np.array_equal(backward, rr.rects(image, rows[::-1], srgb))
    assert not np.array_equal(forward, backward)


@pytest.mark.parametrize("srgb", [False, True], ids=["unorm", "srgb"])
def test_a_long_list(ctx, noise, srgb):
    """300 small overlapping rectangles inside one 16 x 16 area: one tile's list, walked in order"""
    rng = np.random.default_rng(33)
    rows = []
    for i in range(300):
        x0, y0 = (int(v) for v in rng.integers(64 * 40, 64 * 54, 2))
        w, h = (int(v) for v in rng.integers(1, 64 * 4, 2))
        rows.append((x0, y0, min(x0 + w, 64 * 56), min(y0 + h, 64 * 56), tuple(int(v) for v in rng.integers(0, 256, 3)) + ((255, 180, 64, 3)[i % 4],)))
    image = np.ascontiguousarray(noise[:, :128])
    got = _rects(ctx, image, rows, srgb)
    want = rr.rects(image, rows, srgb)
    assert np.array_equal(got, want), np.argwhere(got != want)[:4]
    outside = np.ones(image.shape[:2], bool)
    outside[40:56, 40:56] = False
    assert np.array_equal(got[outside], image[outside]) and not np.array_equal(got, image)


@pytest.mark.parametrize("rect", [(64 * 3 + 17, 64 * 2 + 40, 64 * 80 + 5, 64 * 30 + 9, (200, 90, 20, 255)), (64 * 10, 64 * 10, 64 * 11 - 1, 64 * 40, (0, 255, 9, 99)),
                                  (-100, 64 * 20 + 1, 10 ** 8, 64 * 20 + 33, (255, 255, 255, 1))], ids=["opaque", "thin", "faint"])
def test_consequence_2_on_the_device(ctx, noise, rect):
    """flags = 0: the same bytes as a layer whose alpha plane is k, tinted by fr_layer_shadow without a stage and composited
    by fr_layer_over at o = 255"""
    import torch
    image = np.ascontiguousarray(noise[:48, :128])
    h, w = image.shape[:2]
    layer = np.zeros((h, w, 4), np.uint8)
    layer[..., 3] = rr.coverage(rect, w, h)
    src = torch.from_numpy(layer).to("cuda:0")
    tinted = torch.zeros((h, w, 4), dtype=torch.uint8, device="cuda:0")
    dst = torch.from_numpy(image.copy()).to("cuda:0")
    torch.cuda.synchronize()
    fr.layer_shadow(ctx, src.data_ptr(), w, h, tinted.data_ptr(), w, h, (0, 0, w, h), (0, 0, w, h), (0, 0), 0, 0, 0, rect[4])
    fr.layer_over(ctx, tinted.data_ptr(), w, h, dst.data_ptr(), w, h, fr.make_blits([(0, 0, w, h, 0, 0, 255)]))
    ctx.sync()
    got = _rects(ctx, image, [rect])
    assert np.array_equal(got, dst.cpu().numpy()) and not np.array_equal(got, image)


def test_nothing_to_do(ctx, noise):
    image = np.ascontiguousarray(noise[:50, :128])
    for rows in (None, [], [(640, 640, 640, 1280, (9, 9, 9, 255)), (1280, 640, 640, 1280, (9, 9, 9, 255)), (64 * 128, 0, 64 * 200, 640, (9, 9, 9, 255))],
                 [(0, 0, 64 * 128, 64 * 50, (255, 255, 255, 0)), (100, 100, 5000, 3000, (1, 2, 3, 0))]):
        assert np.array_equal(_rects(ctx, image, rows), image)
        assert np.array_equal(_rects(ctx, image, rows, True), image)


def test_consequence_1_and_refusals(ctx, noise):
    import torch
    image = np.ascontiguousarray(noise[:50, :128])
    for srgb in (False, True):
        got = _rects(ctx, image, [(64 * 8, 64 * 4, 64 * 100, 64 * 40, (17, 250, 3, 255))], srgb)
        want = image.copy()
        want[4:40, 8:100] = (17, 250, 3, 255)
        assert np.array_equal(got, want)
    dst = torch.from_numpy(image.copy()).to("cuda:0")
    torch.cuda.synchronize()
    D, ok = dst.data_ptr(), fr.make_rects([(0, 0, 640, 640, (1, 2, 3, 255))])
    for what, code, args in (("dst NULL", -1, (0, 128, 50)), ("dst not 4-byte aligned", -1, (D + 2, 128, 49)), ("pitch beyond 2^26", -1, (D, (1 << 26) + 1, 0)),
                             ("2^31 rows", -4, (D, 0, 1 << 31))):
        with pytest.raises(fr.FrError) as e:
            fr.layer_rects(ctx, *args, ok)
        assert e.value.code == code, what
    for flags in (2, fr.FR_TEXT_SRGB, fr.FR_TEXT_OVER, 1 << 31):
        with pytest.raises(fr.FrError) as e:
            fr.layer_rects(ctx, D, 128, 50, ok, flags=flags)
        assert e.value.code == -1, flags
    lib = L.load_library()
    assert lib.fr_layer_rects(ctx._h, D, 128, 50, None, 1, 0) == -1 and lib.fr_layer_rects(None, D, 128, 50, L.ptr(ok), 1, 0) == -1
    ctx.sync()
    assert np.array_equal(dst.cpu().numpy(), image)


def test_rgba_fill_rects_method(ctx, noise):
    image = np.ascontiguousarray(noise[:45, :120])
    frame = fr.RGBA(120, 45, image.reshape(-1, 4).copy())
    assert frame.fill_rects([(3.25, 2.5, 80.0, 30.125, (200, 90, 20, 180)), (-4, 9, 7.3, 50, (1, 2, 3, 255))], srgb=True, ctx=ctx) is frame
    rows = [(208, 160, 5120, 1928, (200, 90, 20, 180)), (-256, 576, 467, 3200, (1, 2, 3, 255))]
    assert np.array_equal(frame.as_3d(), rr.rects(image, rows, True))


def test_a_real_line(ctx):
    """draw_text_rgba of a DejaVuSans line at size 32 with decoration_rects drawn under and over it == the twin applied
    around the same text render; the underline changes exactly the rows the metrics give"""
    from font_renderer_amd.text import decoration_rects, draw_text_rgba
    font = load_font("DejaVuSans.ttf", allow_hinted=True)
    text, size, x, y = "Equal quay", 32, 6.25, 40.0
    w, h = 200, 56
    base = np.zeros((h, w, 4), np.uint8)
    base[:] = (20, 30, 40, 255)
    deco = decoration_rects(font, text, size, x, y, underline=(250, 250, 0, 255), strikeout=(255, 0, 0, 160), highlight=(0, 90, 200, 120))
    assert len(deco) == 3
    in64 = [tuple(int(round(64 * v)) for v in r[:4]) + (r[4],) for r in deco]
    _, _, end = font.layout(text, size)
    assert all(r[0] == 400 and r[2] == 400 + end for r in in64)

    def text_over(image):
        im = fr.RGBA(w, h, image.reshape(-1, 4).copy())
        draw_text_rgba(im, font, text, size, x, y, color=(255, 255, 255, 255), over=True, ctx=ctx)
        return im

    got = fr.RGBA(w, h, base.reshape(-1, 4).copy()).fill_rects(deco[:1], ctx=ctx)
    got = text_over(got.as_3d()).fill_rects(deco[1:], ctx=ctx).as_3d()
    lettered = text_over(rr.rects(base, in64[:1])).as_3d()
    want = rr.rects(lettered, in64[1:])
    assert np.array_equal(got, want), np.argwhere(got != want)[:4]
    assert not np.array_equal(lettered, rr.rects(base, in64[:1]))
    # the underline alone: rows 40 + 130 / 64 .. 40 + 220 / 64 of DejaVuSans at 32 pixels per 2048 units
    top, bottom = font.decoration(size, fr.FR_DECOR_UNDERLINE)
    assert (top, bottom) == (130, 220)
    under = fr.RGBA(w, h, lettered.reshape(-1, 4).copy()).fill_rects(deco[1:2], ctx=ctx).as_3d()
    changed = np.flatnonzero((under != lettered).any(axis=(1, 2)))
    assert changed.tolist() == list(range((64 * 40 + top) // 64, -(-(64 * 40 + bottom) // 64))) == [42, 43]

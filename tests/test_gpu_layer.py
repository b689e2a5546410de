"""fr_layer_over and fr_layer_unpremultiply on the GPU (include/fr_raster.h).  The expected image never comes from the code
under test: it is the numpy twin of the definition (tests/layer_ref.py, itself held to exact fractions and to the
header's consequences by tests/test_layer_ref.py), the host function fr_rgba_unpremultiply, or a text plan rendered with
FR_TEXT_LOAD.  Destinations are noise or sentinel-filled with guard rows around them, and whole arrays are compared, so a
byte written outside a clipped rectangle fails; the layer is compared with its copy afterwards."""
import numpy as np
import pytest

import font_renderer_amd as fr
import layer_ref as lr
from fixtures import load_font
from font_renderer_amd import _lib as L
from layer_gpu import SENT, Guarded, premultiplied

pytestmark = pytest.mark.gpu
OPACITIES = (0, 1, 2, 127, 128, 129, 253, 254, 255)
DEST_C = (0, 1, 127, 254, 255)


def _over(ctx, layer, image, blits, srgb=False, src_skip=0, dst_skip=0):
    """fr_layer_over of `layer` (rows, stride, 4) over a guarded device copy of `image` -> (image after, the layer after).
    src_skip / dst_skip: pixels the device arrays are moved by, to leave the 16-byte grid."""
    d = Guarded(image, layer, dst_skip, src_skip)
    fr.layer_over(ctx, d.src, layer.shape[1], layer.shape[0], d.dst, image.shape[1], image.shape[0], blits, srgb)
    return d.result(ctx), d.layer_after


@pytest.fixture(scope="module")
def domain():
    """every (s_c, s_a, d_c), three triples to a pixel: row s_a, combination i = 256 s_c + d_c in channel i mod 3 of pixel
    i div 3; the destination's alpha is the column modulo 256, so every (s_a, d_a) occurs too.  Widths are padded to a
    multiple of four with zero pixels."""
    i = np.arange(65538) % 65536
    s_c, d_c = (i >> 8).reshape(-1, 3), (i & 255).reshape(-1, 3)
    w = (s_c.shape[0] + 3) // 4 * 4
    layer, image = np.zeros((256, w, 4), np.uint8), np.zeros((256, w, 4), np.uint8)
    layer[:, :s_c.shape[0], :3] = s_c
    layer[:, :s_c.shape[0], 3] = np.arange(256)[:, None]
    image[:, :s_c.shape[0], :3] = d_c
    image[..., 3] = np.arange(w) % 256
    return layer, image


@pytest.mark.parametrize("srgb", [False, True], ids=["unorm", "srgb"])
def test_every_triple_at_full_opacity(ctx, domain, srgb):
    """the OPACITY = 0 instance over the whole domain of its arithmetic, the clamp included (s_c > s_a occurs)"""
    layer, image = domain
    got, layer_after = _over(ctx, layer, image, fr.make_blits([(0, 0, layer.shape[1], 256, 0, 0, 255)]), srgb)
    want = lr.over(layer, image, 255, srgb)
    assert np.array_equal(got, want), np.argwhere(got != want)[:4]
    assert np.array_equal(layer_after, layer)


@pytest.mark.parametrize("srgb", [False, True], ids=["unorm", "srgb"])
def test_every_source_pixel_at_the_edge_opacities(ctx, srgb):
    """the OPACITY = 1 instance: every (s_c, s_a) and every (s_a, d_a) at o in OPACITIES over d_c in DEST_C, as 45 blits
    of one call (o = 0 launches no tile, o = 255 runs in the opacity instance)"""
    v = np.arange(256)
    layer = np.zeros((256, 256, 4), np.uint8)
    layer[..., 0], layer[..., 1], layer[..., 2] = v[None, :], (v[None, :] + 85) % 256, 255 - v[None, :]
    layer[..., 3] = v[:, None]
    image = np.zeros((256 * len(OPACITIES), 256 * len(DEST_C), 4), np.uint8)
    image[..., 3] = np.arange(image.shape[1])[None, :] % 256
    for k, d in enumerate(DEST_C):
        image[:, 256 * k:256 * (k + 1), :3] = d
    blits = fr.make_blits([(0, 0, 256, 256, 256 * k, 256 * j, o) for j, o in enumerate(OPACITIES) for k in range(len(DEST_C))])
    got, layer_after = _over(ctx, layer, image, blits, srgb)
    want = lr.composite(layer, image, blits.tolist(), srgb)
    assert np.array_equal(got[..., 3], want[..., 3]), "alpha"
    assert np.array_equal(got, want), np.argwhere(got != want)[:4]
    assert np.array_equal(got[:256], image[:256])                   # o = 0: byte-identical
    assert np.array_equal(layer_after, layer)


GEOMETRY = {
    "negative_offsets": [(0, 0, 97, 41, -5, -7, 255)],
    "partly_outside_right_bottom": [(3, 2, 94, 39, 100, 30, 255)],
    "wholly_outside": [(0, 0, 10, 10, 131, 0, 255), (0, 0, 10, 10, 5, -10, 255), (0, 0, 10, 10, -2 ** 31, 2 ** 31 - 1, 255)],
    "ragged_widths": [(0, 0, 1, 5, 8, 1, 255), (1, 0, 3, 17, 3, 8, 255), (2, 3, 63, 4, 20, 0, 255), (5, 9, 64, 7, 17, 30, 255),
                      (7, 11, 65, 3, 40, 40, 255)],
    "unaligned_src_x": [(5, 0, 40, 10, 8, 0, 255), (6, 0, 40, 10, 10, 20, 255), (1, 1, 96, 9, 0, 38, 255)],
    "touching_blits_and_opacities": [(0, 0, 20, 10, 10, 10, 255), (20, 0, 20, 10, 30, 10, 128), (0, 10, 40, 5, 10, 20, 1),
                                     (40, 0, 57, 41, 60, 5, 254), (0, 0, 30, 12, 0, 30, 0)],
    "whole_layer": [(0, 0, 97, 41, 16, 4, 255)],
}


@pytest.fixture(scope="module")
def small():
    """the 97 x 41 layer in rows of 97 pixels, and the same pixels in rows of 100 (three more columns of other pixels)"""
    rng = np.random.default_rng(7)
    layer = premultiplied(rng, (41, 97))
    return layer, np.concatenate([layer, premultiplied(rng, (41, 3))], 1)


@pytest.mark.parametrize("srgb", [False, True], ids=["unorm", "srgb"])
@pytest.mark.parametrize("stride,wide,src_skip,dst_skip", [(131, 0, 0, 0), (132, 0, 0, 0), (132, 1, 0, 0), (132, 1, 1, 0), (132, 1, 0, 3)],
                         ids=["rows131", "rows132_layer97", "rows132_layer100", "src_off_grid", "dst_off_grid"])
@pytest.mark.parametrize("case", sorted(GEOMETRY))
def test_geometry(ctx, small, case, stride, wide, src_skip, dst_skip, srgb):
    """a 97 x 41 layer into a sentinel-filled 130 x 50 destination in rows of `stride` pixels: rows of 131 take the
    pixel-by-pixel path, rows of 132 the 16-byte path with ragged edges, for the layer too when its rows are 100 pixels
    and its column matches the destination's modulo 4"""
    layer = small[wide]
    image = np.full((50, stride, 4), SENT, np.uint8)
    blits = fr.make_blits(GEOMETRY[case])
    got, layer_after = _over(ctx, layer, image, blits, srgb, src_skip, dst_skip)
    want = lr.composite(layer, image, GEOMETRY[case], srgb)
    assert np.array_equal(got, want), (case, np.argwhere(got != want)[:4])
    assert np.array_equal(layer_after, layer)


@pytest.mark.parametrize("dx,dy", [(1, 0), (3, 2), (4, 5), (30, 7)])
def test_translation(ctx, small, dx, dy):
    """the same blit at (dx, dy) and at (0, 0) over a uniform image differ by exactly that shift"""
    layer = small[0]
    image = np.zeros((60, 132, 4), np.uint8)
    image[:] = (40, 90, 20, 200)
    at0, _ = _over(ctx, layer, image, fr.make_blits([(0, 0, 97, 41, 0, 0, 200)]))
    moved, _ = _over(ctx, layer, image, fr.make_blits([(0, 0, 97, 41, dx, dy, 200)]))
    want = image.copy()
    want[dy:dy + 41, dx:dx + 97] = at0[:41, :97]
    assert np.array_equal(moved, want)
    assert not np.array_equal(at0, image)


@pytest.mark.parametrize("flags", [0, fr.FR_TEXT_SRGB, fr.FR_TEXT_BGRA, fr.FR_TEXT_SRGB | fr.FR_TEXT_BGRA], ids=["rgba", "srgb", "bgra", "srgb_bgra"])
def test_a_text_layer_over_a_frame_is_the_load_render(ctx, flags):
    """consequence 5: FR_TEXT_OVER, n = 1, opaque colours over clear (0, 0, 0, 0), composited at (0, 0) with o = 255 over
    noise == the same plan with FR_TEXT_LOAD on that noise, byte for byte"""
    import torch
    from font_renderer_amd.text import _line
    font = load_font("DejaVuSans.ttf", allow_hinted=True)
    text = "Layer fjord, quay!"
    gs, places, runs, w, h = _line(font, text, 19)
    rng = np.random.default_rng(3)
    cols = rng.integers(0, 256, (len(places), 4)).astype(np.uint8)
    cols[:, 3] = 255
    frame = rng.integers(0, 256, (h, w, 4)).astype(np.uint8)
    dgs = fr.DeviceGlyphSet(ctx, gs)
    try:
        out = {}
        for name, extra, start in (("layer", 0, np.zeros_like(frame)), ("load", fr.FR_TEXT_LOAD, frame)):
            plan = fr.TextPlanRGBA(dgs, places, cols, runs, [(0, 0, 0, 0)], 1, fr.FR_SAMPLE_CENTER, flags | fr.FR_TEXT_OVER | extra)
            buf = torch.from_numpy(start.copy()).to("cuda:0")
            torch.cuda.synchronize()
            plan.render(buf.data_ptr(), w, h)
            ctx.sync()
            out[name] = buf.cpu().numpy()
            plan.close()
    finally:
        dgs.close()
    assert out["layer"][..., 3].max() == 255 and (out["layer"][..., 3] == 0).any()
    got, _ = _over(ctx, out["layer"], frame, fr.make_blits([(0, 0, w, h, 0, 0, 255)]), bool(flags & fr.FR_TEXT_SRGB))
    assert np.array_equal(got, out["load"]), np.argwhere(got != out["load"])[:4]
    assert not np.array_equal(got, frame)


@pytest.mark.parametrize("srgb", [False, True], ids=["unorm", "srgb"])
def test_unpremultiply_is_the_host_function(ctx, srgb):
    """every (c, a) in one 256 x 256 image, and a strided window off the 16-byte grid inside a sentinel-filled image"""
    import torch
    v = np.arange(256)
    c, a = np.meshgrid(v, v, indexing="ij")
    px = np.stack([c, 255 - c, (c * 7 + a) % 256, a], -1).astype(np.uint8)
    want = fr.RGBA(256, 256, px.reshape(-1, 4).copy()).unpremultiply(srgb).data.reshape(px.shape)
    buf = torch.from_numpy(px.copy()).to("cuda:0")
    torch.cuda.synchronize()
    fr.layer_unpremultiply(ctx, buf.data_ptr(), 256, 256, 256, srgb)
    ctx.sync()
    assert np.array_equal(buf.cpu().numpy(), want)
    assert np.array_equal(fr.RGBA(256, 256, px.reshape(-1, 4).copy()).unpremultiply(srgb, device=True, ctx=ctx).data.reshape(px.shape), want)
    # a 97 x 41 window at (3, 2) of a 50-row image in rows of 131
    rng = np.random.default_rng(11)
    image = np.full((50, 131, 4), SENT, np.uint8)
    image[2:43, 3:100] = premultiplied(rng, (41, 97))
    win = np.ascontiguousarray(image[2:43, 3:100]).reshape(-1, 4)
    want = image.copy()
    want[2:43, 3:100] = fr.RGBA(97, 41, win).unpremultiply(srgb).data.reshape(41, 97, 4)
    buf = torch.from_numpy(image.copy()).to("cuda:0")
    torch.cuda.synchronize()
    fr.layer_unpremultiply(ctx, buf.data_ptr() + 4 * (2 * 131 + 3), 131, 97, 41, srgb)
    ctx.sync()
    assert np.array_equal(buf.cpu().numpy(), want)


def test_rgba_over_method(ctx, small):
    layer = fr.RGBA(97, 41, small[0].reshape(-1, 4).copy())
    frame = fr.RGBA(120, 45, premultiplied(np.random.default_rng(5), (45, 120)).reshape(-1, 4))
    before = frame.data.reshape(45, 120, 4).copy()
    assert frame.over(layer, x=-4, y=9, opacity=77, srgb=True, ctx=ctx) is frame
    assert np.array_equal(frame.as_3d(), lr.composite(small[0], before, [(0, 0, 97, 41, -4, 9, 77)], True))


def test_refusals_leave_the_destination_untouched(ctx, small):
    """every refusal of the header through the C ABI: its code, and not a byte of the destination changed"""
    import torch
    layer = small[0]
    src = torch.from_numpy(layer.copy()).to("cuda:0")
    image = np.full((50, 132, 4), SENT, np.uint8)
    dst = torch.from_numpy(image.copy()).to("cuda:0")
    torch.cuda.synchronize()
    S, D = src.data_ptr(), dst.data_ptr()
    ok = [(0, 0, 10, 10, 0, 0, 255)]
    cases = {
        "opacity 256": (-1, (S, 97, 41, D, 132, 50, [(0, 0, 10, 10, 0, 0, 256)])),
        "source rectangle one pixel out": (-1, (S, 97, 41, D, 132, 50, [(88, 0, 10, 10, 0, 0, 255)])),
        "source rectangle one row out": (-1, (S, 97, 41, D, 132, 50, [(0, 32, 10, 10, 0, 0, 255)])),
        "blits overlap by one pixel": (-1, (S, 97, 41, D, 132, 50, [(0, 0, 20, 10, 10, 10, 255), (20, 0, 20, 10, 29, 19, 255)])),
        "the images alias": (-1, (D, 132, 50, D, 132, 50, ok)),
        "the images alias in their last bytes": (-1, (D + 4 * 132 * 49, 97, 41, D, 132, 50, ok)),
        "src not 4-byte aligned": (-1, (S + 2, 97, 40, D, 132, 50, ok)),
        "dst not 4-byte aligned": (-1, (S, 97, 41, D + 1, 132, 49, ok)),
        "src NULL": (-1, (0, 97, 41, D, 132, 50, ok)),
        "dst NULL": (-1, (S, 97, 41, 0, 132, 50, ok)),
        "pitch beyond 2^26": (-1, (S, 97, 41, D, (1 << 26) + 1, 0, ok)),
        "2^31 rows": (-4, (S, 97, 41, D, 0, 1 << 31, ok)),
    }
    for what, (code, (s, ss, sr, d, ds, dr, rows)) in cases.items():
        with pytest.raises(fr.FrError) as e:
            fr.layer_over(ctx, s, ss, sr, d, ds, dr, fr.make_blits(rows))
        assert e.value.code == code, (what, str(e.value))
    for flags in (2, fr.FR_TEXT_SRGB, fr.FR_TEXT_OVER, 1 << 31):
        with pytest.raises(fr.FrError) as e:
            fr.layer_over(ctx, S, 97, 41, D, 132, 50, fr.make_blits(ok), flags=flags)
        assert e.value.code == -1, flags
    with pytest.raises(fr.FrError) as e:                               # NULL blits with a count
        L.check(L.load_library().fr_layer_over(ctx._h, S, 97, 41, D, 132, 50, None, 1, 0))
    assert e.value.code == -1
    fr.layer_over(ctx, S, 97, 41, D, 132, 50, None)                    # n_blits = 0: valid, launches nothing
    fr.layer_over(ctx, S, 97, 41, D, 132, 50, fr.make_blits([(500, 500, 0, 3, 0, 0, 255)]))      # 0 x anything: valid
    for w, h, stride, off, code in ((133, 1, 132, 0, -1), (10, 10, 132, 2, -1), (10, 10, (1 << 26) + 1, 0, -1)):
        with pytest.raises(fr.FrError) as e:
            fr.layer_unpremultiply(ctx, D + off, stride, w, h)
        assert e.value.code == code
    ctx.sync()
    assert np.array_equal(dst.cpu().numpy(), image) and np.array_equal(src.cpu().numpy(), layer)

"""fr_layer_mask on the GPU (include/fr_raster.h).  The expected image never comes from the code under test: it is the numpy
twin of the definition (tests/layer_mask_ref.py, itself held to a brute force and to the header's consequences by
tests/test_layer_mask_ref.py), another call's twin, or another device call where a consequence names one.  Destinations are
noise or sentinel-filled with guard rows around them, and whole arrays are compared, so a byte written outside a clipped
rectangle fails; the layer and the mask are compared with their copies afterwards."""
import itertools

import numpy as np
import pytest

import font_renderer_amd as fr
import layer_mask_ref as mr
import layer_outline_ref as orf
import layer_rects_ref as rr
import layer_ref as lr
import text_gpu as tg
from fixtures import load_font
from font_renderer_amd import _lib as L
from layer_gpu import SENT, Guarded, premultiplied

pytestmark = pytest.mark.gpu
SPACES = pytest.mark.parametrize("srgb", [False, True], ids=["unorm", "srgb"])
KINDS = pytest.mark.parametrize("plane", [False, True], ids=["layer_mask", "plane"])
DEST_C = (0, 1, 127, 254, 255)


class Mask:
    """a device copy of `mask`, (rows, stride, 4) pixels or a (rows, pitch) plane of bytes, moved by `skip` elements to leave
    its grid, between sentinel elements; ptr is the device address to call with"""

    def __init__(self, mask, skip=0):
        import torch
        self.mask, self.skip = mask, skip
        unit = (4,) if mask.ndim == 3 else ()
        pad = np.full((skip,) + unit, SENT, np.uint8)
        self._dev = torch.from_numpy(np.concatenate([pad, mask.reshape((-1,) + unit), np.full((8,) + unit, SENT, np.uint8)])).to("cuda:0")
        self.ptr = self._dev.data_ptr() + skip * (4 if unit else 1)
        torch.cuda.synchronize()

    def check(self):
        got = self._dev.cpu().numpy()
        n = self.mask.shape[0] * self.mask.shape[1]
        assert (got[:self.skip] == SENT).all() and (got[self.skip + n:] == SENT).all() and np.array_equal(got[self.skip:self.skip + n].reshape(self.mask.shape), self.mask), \
            "the mask was written"


def _run(ctx, layer, mask, image, blits, srgb=False, erase=False, src_skip=0, mask_skip=0, dst_skip=0):
    """fr_layer_mask of `layer` (None when erasing) through `mask` over a guarded device copy of `image` -> the image after;
    the layer and the mask are checked against their copies"""
    d = Guarded(image, None if erase else layer, dst_skip, src_skip)
    k = Mask(mask, mask_skip)
    fr.layer_mask(ctx, None if erase else d.src, 0 if erase else layer.shape[1], 0 if erase else layer.shape[0], k.ptr, mask.shape[1], mask.shape[0],
                  d.dst, image.shape[1], image.shape[0], fr.make_mask_blits(blits), srgb, mask.ndim == 2, erase)
    got = d.result(ctx)
    k.check()
    return got


def _as_layer(plane, rng=None):
    """a layer mask whose alpha bytes are the plane's, its colour bytes anything"""
    out = np.zeros(plane.shape + (4,), np.uint8) if rng is None else rng.integers(0, 256, plane.shape + (4,)).astype(np.uint8)
    out[..., 3] = plane
    return out


def _check(ctx, layer, mask, image, blits, srgb=False, erase=False, **skips):
    got = _run(ctx, layer, mask, image, blits, srgb, erase, **skips)
    want = mr.composite(None if erase else layer, mask, image, blits, srgb, erase)
    assert np.array_equal(got, want), (blits, skips, np.argwhere(got != want)[:4])
    return got


# ---- the arithmetic over its domain ------------------------------------------------------------------------------------------
@SPACES
@KINDS
@pytest.mark.parametrize("invert", [0, 1], ids=["through", "inverted"])
def test_every_k_and_o(ctx, srgb, plane, invert):
    """256 blits of 256 x 1, row y at opacity y, mask column = k, an opaque white layer over black: every (k, o) -> t"""
    layer = np.full((256, 256, 4), 255, np.uint8)
    k = np.broadcast_to(np.arange(256, dtype=np.uint8), (256, 256)).copy()
    image = np.zeros((256, 256, 4), np.uint8)
    image[..., 3] = 255
    blits = [(0, y, 256, 1, 0, y, 0, y, y, invert) for y in range(256)]
    got = _check(ctx, layer, k if plane else _as_layer(k, np.random.default_rng(1)), image, blits, srgb)
    assert np.array_equal(got[0], image[0])                      # o = 0: byte-identical
    if not srgb:                                                 # white over black at t is (t, t, t, 255)
        assert np.array_equal(got[..., 0], mr.t_of(k, np.arange(256)[:, None], bool(invert)))


@SPACES
def test_every_source_byte_at_every_t(ctx, srgb):
    """every (s_c, t) under s_a = 255 (upper half) and every (s_a, t) with a premultiplied colour (lower half), t down the
    rows from the mask at o = 255, over d_c in DEST_C and every d_a"""
    v = np.arange(256)
    layer = np.zeros((512, 256, 4), np.uint8)
    layer[:256, :, 0], layer[:256, :, 1], layer[:256, :, 2], layer[:256, :, 3] = v[None, :], (v[None, :] + 85) % 256, 255 - v[None, :], 255
    layer[256:, :, 0], layer[256:, :, 1], layer[256:, :, 2], layer[256:, :, 3] = v[None, :], v[None, :] // 2, (v[None, :] * 3) // 4, v[None, :]
    mask = np.broadcast_to(np.arange(256, dtype=np.uint8)[:, None], (256, 256)).copy()
    image = np.zeros((512, 256 * len(DEST_C), 4), np.uint8)
    image[..., 3] = (np.arange(image.shape[1])[None, :] * 7 + np.arange(512)[:, None]) % 256
    for j, d in enumerate(DEST_C):
        image[:, 256 * j:256 * (j + 1), :3] = d
    blits = [(0, 256 * half, 256, 256, 256 * j, 256 * half, 0, 0, 255, 0) for half in (0, 1) for j in range(len(DEST_C))]
    got = _check(ctx, layer, mask, image, blits, srgb)
    assert np.array_equal(got[0], image[0]) and np.array_equal(got[256], image[256])      # t = 0


@pytest.fixture(scope="module")
def domain():
    """the (s_c, s_a, d_c) domain of tests/test_gpu_layer.py: row s_a, combination i = 256 s_c + d_c in channel i mod 3 of
    pixel i div 3, the destination's alpha the column modulo 256; with the fr_layer_over twin of both spaces, computed once"""
    i = np.arange(65538) % 65536
    s_c, d_c = (i >> 8).reshape(-1, 3), (i & 255).reshape(-1, 3)
    w = (s_c.shape[0] + 3) // 4 * 4
    layer, image = np.zeros((256, w, 4), np.uint8), np.zeros((256, w, 4), np.uint8)
    layer[:, :s_c.shape[0], :3] = s_c
    layer[:, :s_c.shape[0], 3] = np.arange(256)[:, None]
    image[:, :s_c.shape[0], :3] = d_c
    image[..., 3] = np.arange(w) % 256
    return layer, image, {srgb: lr.over(layer, image, 255, srgb) for srgb in (False, True)}


@pytest.mark.parametrize("srgb,plane", [(False, True), (True, False)], ids=["unorm_plane", "srgb_layer_mask"])
def test_the_domain_under_a_full_mask_is_fr_layer_over(ctx, domain, srgb, plane):
    """an all-255 mask leaves fr_layer_over's bytes, the clamp included (s_c > s_a occurs)"""
    layer, image, want = domain
    full = np.full(layer.shape[:2], 255, np.uint8)
    got = _run(ctx, layer, full if plane else _as_layer(full), image, [(0, 0, layer.shape[1], 256, 0, 0, 0, 0, 255, 0)], srgb)
    assert np.array_equal(got, want[srgb]), np.argwhere(got != want[srgb])[:4]


@SPACES
@KINDS
def test_erase_over_its_domain(ctx, srgb, plane):
    """every (d_c, t) and every (d_a, t): the destination's bytes across the columns, t down the rows"""
    v = np.arange(256)
    image = np.zeros((256, 256, 4), np.uint8)
    image[..., 0], image[..., 1], image[..., 2], image[..., 3] = v[None, :], (v[None, :] + 85) % 256, 255 - v[None, :], v[None, :]
    mask = np.broadcast_to(np.arange(256, dtype=np.uint8)[:, None], (256, 256)).copy()
    got = _check(ctx, None, mask if plane else _as_layer(mask), image, [(0, 0, 256, 256, 0, 0, 0, 0, 255, 0)], srgb, True)
    assert np.array_equal(got[0], image[0]) and not got[255].any()              # t = 0 and t = 255
    assert (got[..., 3] <= image[..., 3]).all()
    inv = _check(ctx, None, mask if plane else _as_layer(mask), image, [(0, 0, 256, 256, 0, 0, 0, 0, 255, 1)], srgb, True)
    assert np.array_equal(inv, got[::-1])


# ---- geometry ----------------------------------------------------------------------------------------------------------------
# the GEOMETRY cases of tests/test_gpu_layer.py as (src_x, src_y, w, h, dst_x, dst_y, opacity, invert), and three of this call
GEOMETRY = {
    "negative_offsets": [(0, 0, 97, 41, -5, -7, 255, 0)],
    "partly_outside_right_bottom": [(3, 2, 94, 39, 100, 30, 255, 1)],
    "wholly_outside": [(0, 0, 10, 10, 131, 0, 255, 0), (0, 0, 10, 10, 5, -10, 255, 0), (0, 0, 10, 10, -2 ** 31, 2 ** 31 - 1, 255, 1)],
    "ragged_widths": [(0, 0, 1, 5, 8, 1, 255, 0), (1, 0, 3, 17, 3, 8, 255, 1), (2, 3, 63, 4, 20, 0, 255, 0), (5, 9, 64, 7, 17, 30, 255, 0),
                      (7, 11, 65, 3, 40, 40, 255, 1)],
    "unaligned_src_x": [(5, 0, 40, 10, 8, 0, 255, 0), (6, 0, 40, 10, 10, 20, 255, 0), (1, 1, 96, 9, 0, 38, 255, 0)],
    "touching_blits_inverts_and_opacities": [(0, 0, 20, 10, 10, 10, 255, 0), (20, 0, 20, 10, 30, 10, 128, 1), (0, 10, 40, 5, 10, 20, 1, 0),
                                             (40, 0, 57, 41, 60, 5, 254, 1), (0, 0, 30, 12, 0, 30, 0, 1), (0, 15, 40, 5, 10, 25, 200, 1)],
    "whole_layer": [(0, 0, 97, 41, 16, 4, 255, 0)],
}


@pytest.fixture(scope="module")
def small():
    """the 97 x 41 layer in rows of 97 and of 100 pixels, and a 100 x 44 mask (three columns and rows to move about in) as a
    layer and as a plane, in rows of 100 and 103"""
    rng = np.random.default_rng(7)
    layer = premultiplied(rng, (41, 97))
    plane = rng.integers(0, 256, (44, 100)).astype(np.uint8)
    plane[rng.integers(0, 4, plane.shape) == 0] = 0
    plane[rng.integers(0, 4, plane.shape) == 0] = 255
    return {"layer": layer, "layer100": np.concatenate([layer, premultiplied(rng, (41, 3))], 1), "plane": plane,
            "plane103": np.concatenate([plane, rng.integers(0, 256, (44, 3)).astype(np.uint8)], 1)}


@SPACES
@KINDS
@pytest.mark.parametrize("stride", [131, 132])
@pytest.mark.parametrize("mask_x", [0, 1, 2, 3])
def test_geometry(ctx, small, stride, mask_x, plane, srgb):
    """a 97 x 41 layer into a sentinel-filled 50-row destination in rows of `stride` pixels, the mask's window moved off the
    grid by mask_x; composite and erase"""
    mask = small["plane"] if plane else _as_layer(small["plane"])
    image = np.full((50, stride, 4), SENT, np.uint8)
    for case, rows in GEOMETRY.items():
        blits = [r[:6] + (r[0] + mask_x, r[1] + mask_x % 2, r[6], r[7]) for r in rows]
        _check(ctx, small["layer100"], mask, image, blits, srgb)
        _check(ctx, None, mask, image, blits, srgb, True)


@SPACES
@KINDS
@pytest.mark.parametrize("erase", [False, True], ids=["composite", "erase"])
def test_the_eight_vector_path_combinations(ctx, small, plane, srgb, erase):
    """layer, mask and destination each on the 16-byte grid or moved 1 - 3 elements off it"""
    mask = small["plane"] if plane else _as_layer(small["plane"], np.random.default_rng(3))
    image = premultiplied(np.random.default_rng(4), (50, 132))
    blits = [(0, 0, 97, 41, 16, 4, 0, 0, 255, 0), (4, 0, 40, 5, 0, 45, 8, 39, 100, 1)]
    for n, (s, k, d) in enumerate(itertools.product((0, 1), repeat=3)):
        _check(ctx, small["layer100"], mask, image, blits, srgb, erase, src_skip=s * (1 + n % 3), mask_skip=k * (1 + (n + 1) % 3), dst_skip=d * (1 + (n + 2) % 3))


@SPACES
def test_a_plane_at_every_byte_offset_and_pitch(ctx, small, srgb):
    """the plane's pointer at byte offsets 0 - 3 and its pitch w .. w + 3: the 4-byte loads only where pointer + pitch +
    column allow, and never a byte outside the plane"""
    image = premultiplied(np.random.default_rng(5), (50, 132))
    rng = np.random.default_rng(6)
    for off, extra in itertools.product(range(4), range(4)):
        plane = np.concatenate([small["plane"], rng.integers(0, 256, (44, extra)).astype(np.uint8)], 1)
        blits = [(0, 0, 97, 41, 8, 2, (4 - off) % 4, 1, 255, 0), (0, 0, 30, 6, 100, 44, 70 + extra, 38, 255, 1)]
        _check(ctx, small["layer"], plane, image, blits, srgb, mask_skip=off)
        _check(ctx, None, plane, image, blits, srgb, True, mask_skip=off)


@SPACES
@KINDS
def test_a_blit_across_tile_borders(ctx, plane, srgb):
    """300 x 20 from x = 3: two tile columns and two tile rows"""
    rng = np.random.default_rng(8)
    layer, image = premultiplied(rng, (24, 304)), premultiplied(rng, (30, 320))
    k = rng.integers(0, 256, (24, 304)).astype(np.uint8)
    for dx in (3, 4):
        _check(ctx, layer, k if plane else _as_layer(k), image, [(2, 1, 300, 20, dx, 5, 4, 3, 255, 0)], srgb)
        _check(ctx, None, k if plane else _as_layer(k), image, [(2, 1, 300, 20, dx, 5, 4, 3, 255, 1)], srgb, True)


@SPACES
@KINDS
@pytest.mark.parametrize("stride", [131, 132])
def test_zero_and_opaque_groups(ctx, plane, srgb, stride):
    """groups of four t = 0 and of four zero layer pixels beside live ones (neither loaded nor stored), and groups of four
    a' = 255 or t = 255 (stored without the load), on the 16-byte path and pixel by pixel"""
    rng = np.random.default_rng(9)
    layer = premultiplied(rng, (40, 128))
    k = rng.integers(1, 255, (40, 128)).astype(np.uint8)
    grp = rng.integers(0, 4, (40, 32)).repeat(4, 1)             # per group of four: 0 live, 1 zero layer, 2 t = 0, 3 opaque
    layer[grp == 1] = 0
    k[grp == 2] = 0
    k[grp == 3] = 255
    layer[grp == 3, 3] = 255
    layer[:, 64:68] = 0                                          # and single pixels of each kind inside live groups
    k[:, 68:70] = 0
    k[:, 70:72] = 255
    image = premultiplied(np.random.default_rng(10), (44, stride))
    mask = k if plane else _as_layer(k)
    for dx in (0, 2):
        _check(ctx, layer, mask, image, [(0, 0, 128, 40, dx, 2, 0, 0, 255, 0)], srgb)
        _check(ctx, layer, mask, image, [(0, 0, 128, 40, dx, 2, 0, 0, 254, 0)], srgb)
        got = _check(ctx, None, mask, image, [(0, 0, 128, 40, dx, 2, 0, 0, 255, 0)], srgb, True)
        assert not got[2:42, dx:dx + 128][k == 255].any()


# ---- the consequences that name another call, against that call on the device ---------------------------------------------
def _device(ctx, image, call, *others):
    """call(dst, *device addresses of others) on a guarded copy of image -> the image after"""
    import torch
    d = Guarded(image)
    devs = [torch.from_numpy(np.ascontiguousarray(o)).to("cuda:0") for o in others]
    torch.cuda.synchronize()
    call(d.dst, *(t.data_ptr() for t in devs))
    return d.result(ctx)


@pytest.fixture(scope="module")
def scene():
    rng = np.random.default_rng(12)
    return premultiplied(rng, (41, 100)), premultiplied(rng, (50, 132))


@SPACES
def test_consequence_1_against_fr_layer_over(ctx, scene, srgb):
    layer, image = scene
    rows = [(2, 1, 90, 30, -3, 4, 255), (0, 0, 10, 5, 100, 0, 77), (0, 36, 100, 4, 5, 40, 0)]
    want = _device(ctx, image, lambda d, s: fr.layer_over(ctx, s, 100, 41, d, 132, 50, fr.make_blits(rows), srgb), layer)
    assert not np.array_equal(want, image)
    for value, inv in ((255, 0), (0, 1)):
        blits = [r[:6] + (r[0], r[1], r[6], inv) for r in rows]
        assert np.array_equal(_run(ctx, layer, np.full((41, 100), value, np.uint8), image, blits, srgb), want)
        assert np.array_equal(_run(ctx, layer, _as_layer(np.full((41, 100), value, np.uint8)), image, blits, srgb), want)


@SPACES
def test_consequence_4_against_fr_layer_paint(ctx, scene, srgb):
    mask, image = scene
    for colour, o in (((200, 10, 99), 255), ((255, 255, 255), 128), ((0, 7, 250), 1)):
        solid = np.zeros((41, 100, 4), np.uint8)
        solid[:] = colour + (255,)
        grad = fr.make_gradient_linear(0, 0, 64, 0, [(0, colour + (o,))])
        want = _device(ctx, image, lambda d, s: fr.layer_paint(ctx, s, 100, 41, d, 132, 50, grad, (3, 2, 90, 37), (-4, 6), srgb), mask)
        got = _run(ctx, solid, mask, image, [(3, 2, 90, 37, -4, 6, 3, 2, o, 0)], srgb)
        assert np.array_equal(got, want) and not np.array_equal(got, image)


@SPACES
@pytest.mark.parametrize("erase", [False, True], ids=["composite", "erase"])
def test_consequence_5_a_plane_against_a_layer_mask(ctx, scene, srgb, erase):
    layer, image = scene
    mask = premultiplied(np.random.default_rng(13), (44, 103))
    blits = [(1, 1, 90, 35, 2, 3, 5, 6, 200, 0), (0, 0, 8, 4, 120, 44, 0, 0, 255, 1)]
    a = _run(ctx, layer, mask, image, blits, srgb, erase)
    b = _run(ctx, layer, np.ascontiguousarray(mask[..., 3]), image, blits, srgb, erase)
    assert np.array_equal(a, b) and not np.array_equal(a, image)


@SPACES
def test_consequence_6_against_fr_layer_rects(ctx, scene, srgb):
    _, image = scene
    full = np.full((44, 100), 255, np.uint8)
    for o in (255, 128, 3):
        got = _run(ctx, None, full, image, [(0, 0, 90, 40, 4, 2, 3, 1, o, 0)], srgb, True)
        want = _device(ctx, image, lambda d: fr.layer_rects(ctx, d, 132, 50, fr.make_rects([(64 * 4, 64 * 2, 64 * 94, 64 * 42, (0, 0, 0, o))]), srgb))
        assert np.array_equal(got[..., :3], want[..., :3])
        assert np.array_equal(want[2:42, 4:94, 3].astype(int) - got[2:42, 4:94, 3], np.full((40, 90), o))     # the alpha differs by o
        assert (got[..., 3] <= image[..., 3]).all()
    assert not _run(ctx, None, full, image, [(0, 0, 90, 40, 4, 2, 3, 1, 255, 0)], srgb, True)[2:42, 4:94].any()


# ---- end to end: a real font, one stream, no sync between the calls ------------------------------------------------------
def _text_scene(ctx, srgb, text, pad):
    """a DejaVuSans line as a plan that renders a premultiplied layer, and device buffers: the layer, two scratch layers of
    the frame's size and a noise frame `pad` pixels larger than the line on every side"""
    import torch
    from font_renderer_amd.text import _line
    font = load_font("DejaVuSans.ttf", allow_hinted=True)
    gs, places, runs, w, h = _line(font, text, 19)
    cols = tg.colours(len(places), 5, opaque=True)
    dgs = fr.DeviceGlyphSet(ctx, gs)
    plan = fr.TextPlanRGBA(dgs, places, cols, runs, [(0, 0, 0, 0)], 1, fr.FR_SAMPLE_CENTER, fr.FR_TEXT_OVER | (fr.FR_TEXT_SRGB if srgb else 0))
    W, H = (w + 2 * pad + 3) // 4 * 4, h + 2 * pad
    frame = tg.noise((H, W), 9)
    dev = {"text": torch.zeros((h, w, 4), dtype=torch.uint8, device="cuda:0"), "a": torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda:0"),
           "b": torch.full((H, W, 4), SENT, dtype=torch.uint8, device="cuda:0"), "frame": torch.from_numpy(frame.copy()).to("cuda:0")}
    torch.cuda.synchronize()
    return dgs, plan, dev, frame, (w, h, W, H)


@SPACES
def test_text_clipped_to_a_rounded_panel(ctx, srgb):
    """the line rendered as a layer and composited through a rounded panel's alpha: the panel is fr_layer_rects into a cleared
    layer followed by fr_layer_outline (GROW, 5 pixels), read back and fed to the twin; render, mask and composite follow
    each other on the stream with no sync between them"""
    pad = 8
    dgs, plan, dev, frame, (w, h, W, H) = _text_scene(ctx, srgb, "Clipped fjord, quay!", pad)
    # the panel cuts the line: its rounded corners lie inside the text's rectangle
    rect = (64 * (pad + 12), 64 * (pad + 3), 64 * (pad + w - 30), 64 * (pad + h - 4), (255, 255, 255, 255))
    try:
        plan.render(dev["text"].data_ptr(), w, h)
        fr.layer_rects(ctx, dev["a"].data_ptr(), W, H, fr.make_rects([rect]))
        fr.layer_outline(ctx, dev["a"].data_ptr(), W, H, dev["b"].data_ptr(), W, H, (0, 0, W, H), (0, 0, W, H), (0, 0), 80, orf.GROW, (9, 9, 9, 255))
        fr.layer_mask(ctx, dev["text"].data_ptr(), w, h, dev["b"].data_ptr(), W, H, dev["frame"].data_ptr(), W, H,
                      fr.make_mask_blits([(0, 0, w, h, pad, pad, pad, pad, 230, 0)]), srgb)
        ctx.sync()
    finally:
        plan.close()
        dgs.close()
    text, panel, got = dev["text"].cpu().numpy(), dev["b"].cpu().numpy(), dev["frame"].cpu().numpy()
    assert text[..., 3].max() == 255 and (text[..., 3] == 0).any()
    assert np.array_equal(panel, orf.outline_rect(rr.rects(np.zeros((H, W, 4), np.uint8), [rect]), (0, 0, W, H), (W, H), (0, 0), 80, orf.GROW, (9, 9, 9, 255)))
    inside = panel[pad:pad + h, pad:pad + w, 3]
    assert (inside == 0).any() and (inside == 255).any() and ((inside > 0) & (inside < 255)).any()
    want = mr.composite(text, panel, frame, [(0, 0, w, h, pad, pad, pad, pad, 230, 0)], srgb)
    assert np.array_equal(got, want), np.argwhere(got != want)[:4]
    assert not np.array_equal(got, frame) and np.array_equal(got[:, :pad + 7], frame[:, :pad + 7])


@SPACES
def test_skip_ink_underline(ctx, srgb):
    """the route of DESIGN section 9: the underline drawn into a cleared layer, erased through the GROW outline of the text
    layer, composited over the frame, then the text over it; five calls behind the render with no sync"""
    pad = 6
    dgs, plan, dev, frame, (w, h, W, H) = _text_scene(ctx, srgb, "Skip gjpqy ink", pad)
    line = (64 * pad, 64 * (pad + h - 6) + 32, 64 * (pad + w), 64 * (pad + h - 4), (20, 40, 200, 255))
    whole = fr.make_blits([(0, 0, W, H, 0, 0, 255)])
    try:
        plan.render(dev["text"].data_ptr(), w, h)
        fr.layer_rects(ctx, dev["a"].data_ptr(), W, H, fr.make_rects([line]), srgb)
        fr.layer_outline(ctx, dev["text"].data_ptr(), w, h, dev["b"].data_ptr(), W, H, (0, 0, w, h), (0, 0, W, H), (pad, pad), 24, orf.GROW, (0, 0, 0, 255))
        fr.layer_mask(ctx, None, 0, 0, dev["b"].data_ptr(), W, H, dev["a"].data_ptr(), W, H, fr.make_mask_blits([(0, 0, W, H, 0, 0, 0, 0, 255, 0)]), srgb, erase=True)
        fr.layer_over(ctx, dev["a"].data_ptr(), W, H, dev["frame"].data_ptr(), W, H, whole, srgb)
        fr.layer_over(ctx, dev["text"].data_ptr(), w, h, dev["frame"].data_ptr(), W, H, fr.make_blits([(0, 0, w, h, pad, pad, 255)]), srgb)
        ctx.sync()
    finally:
        plan.close()
        dgs.close()
    text, got = dev["text"].cpu().numpy(), dev["frame"].cpu().numpy()
    drawn = rr.rects(np.zeros((H, W, 4), np.uint8), [line], srgb)
    grown = orf.outline_rect(text, (0, 0, w, h), (W, H), (pad, pad), 24, orf.GROW, (0, 0, 0, 255))
    assert np.array_equal(dev["b"].cpu().numpy(), grown)
    under = mr.composite(None, grown, drawn, [(0, 0, W, H, 0, 0, 0, 0, 255, 0)], srgb, True)
    assert np.array_equal(dev["a"].cpu().numpy(), under)
    assert (under[..., 3] < drawn[..., 3]).any() and (under[..., 3] == 255).any(), "the descenders cut the line, and some of it stays"
    want = lr.composite(text, lr.composite(under, frame, whole.tolist(), srgb), [(0, 0, w, h, pad, pad, 255)], srgb)
    assert np.array_equal(got, want), np.argwhere(got != want)[:4]


# ---- the interface ---------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_image_untouched(ctx, small):
    """every refusal of the header through the C ABI: its code, and not a byte of the image, the layer or the mask changed"""
    import torch
    layer, mask = small["layer"], _as_layer(small["plane"])
    image = np.full((50, 132, 4), SENT, np.uint8)
    src, msk, dst = (torch.from_numpy(a.copy()).to("cuda:0") for a in (layer, mask, image))
    torch.cuda.synchronize()
    S, M, D = src.data_ptr(), msk.data_ptr(), dst.data_ptr()
    ok = [(0, 0, 10, 10, 0, 0, 0, 0, 255, 0)]

    def call(s=S, ss=97, sr=41, m=M, ms=100, mrows=44, d=D, ds=132, dr=50, rows=ok, **flags):
        fr.layer_mask(ctx, s, ss, sr, m, ms, mrows, d, ds, dr, fr.make_mask_blits(rows), **flags)

    cases = {
        "opacity 256": (-1, dict(rows=[(0, 0, 10, 10, 0, 0, 0, 0, 256, 0)])),
        "invert 2": (-1, dict(rows=[(0, 0, 10, 10, 0, 0, 0, 0, 255, 2)])),
        "the rectangle one pixel out of the layer": (-1, dict(rows=[(88, 0, 10, 10, 0, 0, 0, 0, 255, 0)])),
        "the rectangle one row out of the layer": (-1, dict(rows=[(0, 32, 10, 10, 0, 0, 0, 0, 255, 0)])),
        "the rectangle one element out of the mask": (-1, dict(rows=[(0, 0, 10, 10, 0, 0, 91, 0, 255, 0)])),
        "the rectangle one row out of the mask": (-1, dict(rows=[(0, 0, 10, 10, 0, 0, 0, 35, 255, 0)])),
        "out of the mask when erasing": (-1, dict(s=None, rows=[(0, 0, 10, 10, 0, 0, 91, 0, 255, 0)], erase=True)),
        "out of the plane": (-1, dict(ms=400, mrows=44, rows=[(0, 0, 10, 10, 0, 0, 0, 35, 255, 0)], plane=True)),
        "blits overlap by one pixel": (-1, dict(rows=[(0, 0, 20, 10, 10, 10, 0, 0, 255, 0), (20, 0, 20, 10, 29, 19, 0, 0, 255, 1)])),
        "the image is the layer": (-1, dict(s=D, ss=132, sr=50)),
        "the image is the mask": (-1, dict(m=D, ms=132, mrows=50)),
        "the image is the mask when erasing": (-1, dict(s=None, m=D, ms=132, mrows=50, erase=True)),
        "the image is the plane's last bytes": (-1, dict(m=D - 4 * 132 * 50 + 4, ms=4 * 132, mrows=50, plane=True)),
        "src not 4-byte aligned": (-1, dict(s=S + 2, sr=40)),
        "mask not 4-byte aligned": (-1, dict(m=M + 2, mrows=43)),
        "dst not 4-byte aligned": (-1, dict(d=D + 1, dr=49)),
        "src NULL": (-1, dict(s=None)),
        "mask NULL": (-1, dict(m=0)),
        "dst NULL": (-1, dict(d=0)),
        "erase with a layer": (-1, dict(erase=True)),
        "dst pitch beyond 2^26": (-1, dict(ds=(1 << 26) + 1, dr=0)),
        "mask pitch beyond 2^26": (-1, dict(ms=(1 << 26) + 1, mrows=0)),
        "src pitch beyond 2^26": (-1, dict(ss=(1 << 26) + 1, sr=0)),
        "2^31 rows of image": (-4, dict(ds=0, dr=1 << 31)),
        "2^31 rows of mask": (-4, dict(ms=0, mrows=1 << 31)),
        "2^31 rows of layer": (-4, dict(ss=0, sr=1 << 31)),
    }
    for what, (code, kw) in cases.items():
        with pytest.raises(fr.FrError) as e:
            call(**kw)
        assert e.value.code == code, (what, str(e.value))
    for flags in (fr.FR_LCD_BGR, 16, fr.FR_TEXT_OVER, 1 << 31):
        with pytest.raises(fr.FrError) as e:
            call(flags=flags)
        assert e.value.code == -1, flags
    lib = L.load_library()
    with pytest.raises(fr.FrError) as e:                               # NULL blits with a count
        L.check(lib.fr_layer_mask(ctx._h, S, 97, 41, M, 100, 44, D, 132, 50, None, 1, 0))
    assert e.value.code == -1
    with pytest.raises(fr.FrError) as e:                               # NULL ctx
        L.check(lib.fr_layer_mask(None, S, 97, 41, M, 100, 44, D, 132, 50, None, 0, 0))
    assert e.value.code == -1
    # the other layer calls refuse the two new flag bits
    for flags in (fr.FR_MASK_PLANE, fr.FR_MASK_ERASE):
        with pytest.raises(fr.FrError) as e:
            fr.layer_over(ctx, S, 97, 41, D, 132, 50, fr.make_blits([(0, 0, 10, 10, 0, 0, 255)]), flags=flags)
        assert e.value.code == -1
    # valid calls that change nothing: no blits, 0 x anything, opacity 0 everywhere, wholly clipped away (that they have no
    # tile, and so launch nothing, is tests/test_layer_mask_tables.py's to show)
    fr.layer_mask(ctx, S, 97, 41, M, 100, 44, D, 132, 50, None)
    call(rows=[(500, 500, 0, 3, 0, 0, 500, 500, 255, 0)])
    call(rows=[(0, 0, 10, 10, 0, 0, 0, 0, 0, 0), (0, 0, 10, 10, 20, 0, 0, 0, 0, 1)])
    call(rows=[(0, 0, 10, 10, 132, 0, 0, 0, 255, 0)])
    call(s=None, rows=[(0, 0, 10, 10, 0, 0, 0, 0, 0, 1)], erase=True)
    ctx.sync()
    assert np.array_equal(dst.cpu().numpy(), image) and np.array_equal(src.cpu().numpy(), layer) and np.array_equal(msk.cpu().numpy(), mask)
    # the layer and the mask may be the same memory
    fr.layer_mask(ctx, S, 97, 41, S, 97, 41, D, 132, 50, fr.make_mask_blits([(0, 0, 97, 41, 3, 3, 0, 0, 255, 0)]))
    ctx.sync()
    assert np.array_equal(dst.cpu().numpy(), mr.composite(layer, layer, image, [(0, 0, 97, 41, 3, 3, 0, 0, 255, 0)]))


def test_rgba_over_masked_and_erase_methods(ctx, small):
    layer = fr.RGBA(97, 41, small["layer"].reshape(-1, 4).copy())
    gray = fr.Gray(100, 44, small["plane"].reshape(-1).copy())
    rgba = fr.RGBA(100, 44, _as_layer(small["plane"]).reshape(-1, 4).copy())
    start = premultiplied(np.random.default_rng(5), (45, 120))
    for mask, arr in ((gray, small["plane"]), (rgba, _as_layer(small["plane"]))):
        frame = fr.RGBA(120, 45, start.reshape(-1, 4).copy())
        assert frame.over_masked(layer, mask, x=-4, y=9, mask_xy=(2, 1), opacity=77, invert=True, srgb=True, ctx=ctx) is frame
        assert np.array_equal(frame.as_3d(), mr.composite(small["layer"], arr, start, [(0, 0, 97, 41, -4, 9, 2, 1, 77, 1)], True))
        frame = fr.RGBA(120, 45, start.reshape(-1, 4).copy())
        assert frame.over_masked(layer, mask, x=5, y=0, mask_xy=(50, 30), ctx=ctx) is frame          # only what the mask covers
        assert np.array_equal(frame.as_3d(), mr.composite(small["layer"], arr, start, [(0, 0, 50, 14, 5, 0, 50, 30, 255, 0)]))
        frame = fr.RGBA(120, 45, start.reshape(-1, 4).copy())
        assert frame.erase(mask, x=30, y=-3, mask_xy=(1, 2), opacity=200, ctx=ctx) is frame
        assert np.array_equal(frame.as_3d(), mr.composite(None, arr, start, [(0, 0, 99, 42, 30, -3, 1, 2, 200, 0)], False, True))
    with pytest.raises(ValueError):
        fr.RGBA(120, 45, start.reshape(-1, 4).copy()).erase(gray, opacity=256, ctx=ctx)

"""Pins the CPU twin of RGBA text plans (tests/text_twin.py) to the consequences the definition states
(include/fr_raster.h), checks the kernel's divide-by-255 shortcut over its whole domain, and decodes the 4-channel QOI
writer with Pillow."""
import io

import numpy as np
import pytest

import text_twin as tw
from fixtures import load_font

STRINGS = ["ffi fj Tf", "Wavy /// fff"]


@pytest.fixture(scope="module")
def italic():
    """two lines of real text, and a third run of glyphs packed so close that their ink overlaps"""
    font = load_font("DejaVuSerif-Italic.ttf")
    gs, places, runs, shape = tw.lines(font, STRINGS + ["WoWfj"], 19, pad=1)
    k0 = int(runs[2]["first"])
    places["pen_x64"][k0:k0 + 5] = places["pen_x64"][k0] + np.array([0, 203, 390, 611, 777])
    return gs, places, runs, shape


def _colors(k, seed, opaque=True):
    rng = np.random.default_rng(seed)
    c = rng.integers(0, 256, (k, 4), dtype=np.int64)
    if opaque:
        c[:, 3] = 255
    return c.astype(np.uint8)


@pytest.mark.parametrize("n,center,fill", [(1, False, False), (2, True, True), (4, True, False), (4, False, True)])
def test_white_on_transparent_is_the_coverage(italic, n, center, fill):
    gs, places, runs, _ = italic
    white = np.full((len(places), 4), 255, np.uint8)
    for run in runs:
        got = tw.rgba_render_run("plain", gs, places, white, run, (0, 0, 0, 0), None, n, center, fill)
        want = tw.render_run("plain", gs, places, run, n, center, fill)
        for ch in range(4):
            assert np.array_equal(got[..., ch], want), (n, center, fill, ch)


def test_opaque_colours_last_instance_wins(italic):
    gs, places, runs, _ = italic
    n = 4
    cols = _colors(len(places), 7)
    clear = np.array([12, 34, 56, 78], np.int64)
    overlaps = 0
    for run in runs:
        w, h = int(run["w"]), int(run["h"])
        # argmax formulation: the index of the last instance that covers each sample, or -1
        last = np.full((h * n, w * n), -1, np.int64)
        overlap = np.zeros((h * n, w * n), np.int64)
        for k, y0, x0, hit in tw.instance_hits("plain", gs, places, run, n, True):
            sl = np.s_[y0 * n:y0 * n + hit.shape[0], x0 * n:x0 * n + hit.shape[1]]
            last[sl] = np.where(hit, k, last[sl])
            overlap[sl] += hit
        overlaps += int((overlap > 1).sum())
        table = np.vstack([cols.astype(np.int64), clear[None, :]])     # index -1: the clear colour
        want = tw.resolve(table[last], n)
        assert np.array_equal(tw.rgba_render_run("plain", gs, places, cols, run, clear, None, n, True), want)
    assert overlaps > 0


def test_alpha_zero_keeps_rgb_and_clears_alpha(italic):
    gs, places, runs, _ = italic
    n = 4
    clear = (10, 200, 30, 200)
    cols = np.zeros((len(places), 4), np.uint8)
    cols[:, :3] = _colors(len(places), 3)[:, :3]                     # any RGB: with A = 0 it must not show
    for run in runs:
        got = tw.rgba_render_run("plain", gs, places, cols, run, clear, None, n, True)
        k = tw.coverage_samples("plain", gs, places, run, n, True).reshape(int(run["h"]), n, int(run["w"]), n).sum(axis=(1, 3))
        for ch in range(3):
            assert (got[..., ch] == clear[ch]).all()
        assert np.array_equal(got[..., 3], ((200 * (n * n - k) + n * n // 2) // (n * n)).astype(np.uint8))
        assert (got[..., 3] == 0).any() and (got[..., 3] == 200).any()


def test_order_matters(italic):
    gs, places, runs, _ = italic
    run = runs[2]
    k0 = int(run["first"])
    # the first two placements of the packed run overlap; swap them (and their colours) and the overlap changes colour
    red, blue = (255, 0, 0, 255), (0, 0, 255, 160)
    cols = np.zeros((len(places), 4), np.uint8)
    cols[k0], cols[k0 + 1] = red, blue
    a = tw.rgba_render_run("plain", gs, places, cols, run, (0, 0, 0, 0), None, 4, True)
    sw = places.copy()
    sw[k0], sw[k0 + 1] = places[k0 + 1], places[k0]
    cols_sw = cols.copy()
    cols_sw[k0], cols_sw[k0 + 1] = cols[k0 + 1], cols[k0]
    b = tw.rgba_render_run("plain", gs, sw, cols_sw, run, (0, 0, 0, 0), None, 4, True)
    assert not np.array_equal(a, b)
    # ... and only where the two instances overlap
    hits = {k: (y0, x0, hit) for k, y0, x0, hit in tw.instance_hits("plain", gs, places, run, 4, True)}
    cover = []
    for k in (k0, k0 + 1):
        y0, x0, hit = hits[k]
        m = np.zeros((int(run["h"]) * 4, int(run["w"]) * 4), bool)
        m[y0 * 4:y0 * 4 + hit.shape[0], x0 * 4:x0 * 4 + hit.shape[1]] = hit
        cover.append(m.reshape(int(run["h"]), 4, int(run["w"]), 4).any(axis=(1, 3)))
    diff = (a != b).any(axis=2)
    assert not (diff & ~(cover[0] & cover[1])).any()


def test_divide_by_255_shortcut_is_exact():
    """text_rgba_kernel (fr_text.hip, blend2): (x + 127) div 255 as (t + (t >> 8)) >> 8, t = x + 128, for every
    x = C*A + c*(255 - A) in [0, 65025]; and two such x in the 16-bit halves of one word do not disturb each other"""
    x = np.arange(65026, dtype=np.uint32)
    t = x + 128
    assert np.array_equal((t + (t >> 8)) >> 8, (x + 127) // 255)
    assert int((t + (t >> 8)).max()) < 1 << 16
    for shift in (0, 1, 12345, 65025):
        hi = np.roll(x, shift)
        w = (x | hi << 16) + np.uint32(0x00800080)
        r = ((w + ((w >> 8) & 0x00ff00ff)) >> 8) & 0x00ff00ff
        assert np.array_equal(r & 0xff, (x + 127) // 255) and np.array_equal(r >> 16, (hi + 127) // 255)
    # every (c, C, A) lands in that domain
    c = np.arange(256, dtype=np.int64)
    assert (c[:, None, None] * c[None, None, :] + c[None, :, None] * (255 - c[None, None, :])).max() == 65025


def _qoi_decode(data):
    from PIL import Image
    im = Image.open(io.BytesIO(data))
    assert im.format == "QOI" and im.mode == "RGBA"
    return np.asarray(im.convert("RGBA"))


@pytest.mark.parametrize("kind", ["random", "runs", "alpha"])
def test_qoi_rgba_decodes_with_pillow(kind):
    from font_renderer_amd import qoi
    rng = np.random.default_rng(11)
    h, w = 37, 53
    if kind == "random":
        a = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    elif kind == "runs":                            # long runs (past 62), small steps (DIFF / LUMA), repeats (INDEX)
        a = np.zeros((h, w, 4), np.uint8)
        a[..., 3] = 255
        a[5:, :, 0] = 40
        a[9:20, 7:30] = (41, 39, 40, 255)
        a[20:30] = rng.integers(0, 4, (10, w, 1), dtype=np.uint8) * np.array([1, 1, 1, 0], np.uint8) + np.array([60, 70, 80, 255], np.uint8)
        a[30:] = np.array([[(1, 2, 3, 255), (200, 100, 50, 255)][(i // 3) % 2] for i in range(w)], np.uint8)
    else:                                           # alpha changes with equal RGB, and equal RGBA after an alpha change
        a = np.zeros((h, w, 4), np.uint8)
        a[..., :3] = (225, 105, 180)
        a[..., 3] = rng.choice([0, 0, 128, 255], (h, w))
    data = qoi.saveRGBA(a)
    assert data[:4] == b"qoif" and data[12] == 4 and data[-8:] == b"\0" * 7 + b"\1"
    assert np.array_equal(_qoi_decode(data), a), kind
    assert len(data) <= 22 + 5 * w * h
    if kind == "runs":
        assert len(data) < a.size // 4

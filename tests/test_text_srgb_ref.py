"""sRGB text plans on the CPU: the library's conversions (fr_srgb_decode / fr_srgb_encode, include/fr_raster.h) against
the binary64 definition for every input, the generated table header against its generator, the kernel's divide-by-255
shortcut over its whole domain, and the CPU twin (tests/text_twin.py) against the consequences the definition
states."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import font_renderer_amd as fr
import text_twin as tw
from fixtures import load_font

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_flag_values():
    assert (fr.FR_TEXT_SRGB, fr.FR_TEXT_BGRA, fr.FR_FILL_CONSISTENT) == (8, 4, 1)


# ---- the tables ---------------------------------------------------------------------------------------------------------
def test_decode_every_byte():
    got = fr.srgb_to_linear16(np.arange(256, dtype=np.uint8))
    assert got.dtype == np.uint16
    want = [math.floor(65535.0 * tw.srgb_decode(v / 255.0) + 0.5) for v in range(256)]
    assert got.tolist() == want
    assert (got[0], got[128], got[255]) == (0, 14146, 65535)
    assert np.array_equal(fr.srgb_to_linear16(np.arange(256, dtype=np.uint8).reshape(16, 16)), got.reshape(16, 16))


def test_encode_every_value():
    L = np.arange(65536)
    got = fr.linear16_to_srgb(L)
    assert got.dtype == np.uint8
    thr = [math.ceil(65535.0 * tw.srgb_decode((k - 0.5) / 255.0)) for k in range(1, 256)]
    want = np.zeros(65536, np.int64)
    for t in thr:                                   # E(L) = #{k : L >= T[k]}
        want[t:] += 1
    assert np.array_equal(got, want)
    assert fr.linear16_to_srgb([32768]).tolist() == [188]             # 50 % of white over black in linear light
    with pytest.raises(ValueError):
        fr.linear16_to_srgb([65536])


def test_tables_are_unambiguous_in_binary64():
    """no rounding of the definition is within reach of binary64 error, so the integer tables are the definition"""
    dv = [65535.0 * tw.srgb_decode(v / 255.0) for v in range(256)]
    assert min(abs(x - math.floor(x) - 0.5) for x in dv) > 1e-3
    tk = [65535.0 * tw.srgb_decode((k - 0.5) / 255.0) for k in range(1, 256)]
    assert min(min(x - math.floor(x), math.ceil(x) - x) for x in tk) > 1e-4
    assert int(np.diff(tw.T).min()) >= 19                          # one threshold at most per 16-value bucket


def test_round_trip_and_monotonic():
    D = fr.srgb_to_linear16(np.arange(256, dtype=np.uint8)).astype(np.int64)
    assert (np.diff(D) > 0).all()
    assert np.array_equal(fr.linear16_to_srgb(D), np.arange(256))
    E = fr.linear16_to_srgb(np.arange(65536)).astype(np.int64)
    assert E[0] == 0 and E[-1] == 255 and set(np.diff(E).tolist()) == {0, 1}
    # round to nearest in the encoded domain: L lies closer (in f^-1) to E(L) / 255 than to its neighbours
    inv = lambda l: np.where(l <= 0.04045 / 12.92, l * 12.92, 1.055 * l ** (1 / 2.4) - 0.055)      # noqa: E731
    enc = inv(np.arange(65536) / 65535.0) * 255.0
    assert (np.abs(enc - E) <= 0.5 + 1e-6).all()


def test_generated_header_is_current(tmp_path):
    """font-renderer_amd/csrc/fr_srgb.hpp is what tools/gen_srgb.py writes"""
    out = tmp_path / "fr_srgb.hpp"
    subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "gen_srgb.py"), str(out)])
    assert out.read_text() == open(os.path.join(ROOT, "font-renderer_amd", "csrc", "fr_srgb.hpp")).read()


def test_conversion_null_arguments():
    lib = fr.load_library()
    assert lib.fr_srgb_decode(None, 0, None) == 0 and lib.fr_srgb_encode(None, 0, None) == 0
    assert lib.fr_srgb_decode(None, 3, None) == -1 and lib.fr_srgb_encode(None, 3, None) == -1


def test_divide_by_255_shortcut_is_exact():
    """text_srgb_kernel (fr_text.hip, div255_24): y div 255 as (y * 0x808081) >> 31 for every y = x + 127,
    x = D[C] * A + D[c] * (255 - A) in [0, 65535 * 255]; and every (C, c, A) lands in that domain"""
    top = 65535 * 255 + 127
    assert top < 1 << 24
    for lo in range(0, top + 1, 1 << 22):
        y = np.arange(lo, min(lo + (1 << 22), top + 1), dtype=np.uint64)
        assert np.array_equal((y * np.uint64(0x808081)) >> np.uint64(31), y // np.uint64(255)), lo
    a = np.arange(256, dtype=np.int64)
    assert (tw.D[-1] * a + tw.D[-1] * (255 - a)).max() == 65535 * 255


# ---- the twin's consequences ----------------------------------------------------------------------------------------
STRINGS = ["ffi fj Tf", "Wavy /// fff"]


@pytest.fixture(scope="module")
def italic():
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


@pytest.mark.parametrize("center,fill", [(False, False), (True, True)])
def test_one_sample_opaque_equals_unorm(italic, center, fill):
    gs, places, runs, _ = italic
    cols = _colors(len(places), 4)
    for run in runs:
        got = tw.rgba_render_run("plain", gs, places, cols, run, (9, 250, 120, 77), None, 1, center, fill, srgb=True)
        assert np.array_equal(got, tw.rgba_render_run("plain", gs, places, cols, run, (9, 250, 120, 77), None, 1, center, fill))


@pytest.mark.parametrize("n,opaque", [(4, False), (2, True), (4, True), (1, False)])
def test_alpha_equals_unorm_and_bgra_swaps(italic, n, opaque):
    gs, places, runs, _ = italic
    cols = _colors(len(places), 10 + n, opaque)
    cols[::4, 3] = 0
    diff = 0
    for run in runs:
        got = tw.rgba_render_run("plain", gs, places, cols, run, (30, 60, 90, 200), None, n, True, srgb=True)
        unorm = tw.rgba_render_run("plain", gs, places, cols, run, (30, 60, 90, 200), None, n, True)
        assert np.array_equal(got[..., 3], unorm[..., 3])
        diff += int((got[..., :3] != unorm[..., :3]).sum())
        b = tw.rgba_render_run("plain", gs, places, cols, run, (30, 60, 90, 200), None, n, True, srgb=True, bgr=True)
        assert np.array_equal(b, got[..., [2, 1, 0, 3]])
        # BGRA is the plan with R and B swapped in every colour
        sw = cols[:, [2, 1, 0, 3]]
        assert np.array_equal(b, tw.rgba_render_run("plain", gs, places, sw, run, (90, 60, 30, 200), None, n, True, srgb=True))
    assert diff > 0 or (n == 1 and opaque)


@pytest.mark.parametrize("n,center,fill", [(1, False, False), (2, True, True), (4, True, False), (4, False, True)])
def test_white_on_transparent_map(italic, n, center, fill):
    gs, places, runs, _ = italic
    white = np.full((len(places), 4), 255, np.uint8)
    for run in runs:
        got = tw.rgba_render_run("plain", gs, places, white, run, (0, 0, 0, 0), None, n, center, fill, srgb=True)
        h, w = int(run["h"]), int(run["w"])
        k = tw.coverage_samples("plain", gs, places, run, n, center, fill).reshape(h, n, w, n).sum(axis=(1, 3))
        want = tw.srgb_encode((65535 * k + n * n // 2) // (n * n))
        for ch in range(3):
            assert np.array_equal(got[..., ch], want)
        assert np.array_equal(got[..., 3], tw.render_run("plain", gs, places, run, n, center, fill))
    if n == 2:      # the map itself: 0, 1, 2, 3, 4 of 4 samples
        assert tw.srgb_encode((65535 * np.arange(5) + 2) // 4).tolist() == [0, 137, 188, 225, 255]


def test_alpha_zero_keeps_rgb_and_last_opaque_wins(italic):
    gs, places, runs, _ = italic
    n, clear = 4, (10, 200, 30, 200)
    cols = _colors(len(places), 3)
    cols[:, 3] = 0
    for run in runs:
        got = tw.rgba_render_run("plain", gs, places, cols, run, clear, None, n, True, srgb=True)
        assert (got[..., :3] == clear[:3]).all()
    cols = _colors(len(places), 8)
    for run in runs:
        w, h = int(run["w"]), int(run["h"])
        last = np.full((h * n, w * n), -1, np.int64)
        for k, y0, x0, hit in tw.instance_hits("plain", gs, places, run, n, True):
            sl = np.s_[y0 * n:y0 * n + hit.shape[0], x0 * n:x0 * n + hit.shape[1]]
            last[sl] = np.where(hit, k, last[sl])
        table = np.vstack([cols.astype(np.int64), np.array(clear, np.int64)[None, :]])
        assert np.array_equal(tw.rgba_render_run("plain", gs, places, cols, run, clear, None, n, True, srgb=True), tw.srgb_resolve(table[last], n))

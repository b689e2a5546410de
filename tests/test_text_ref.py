"""Pins the CPU twin of text runs (tests/text_twin.py) to the oracle: one instance with a whole-pixel pen is the
ordinary renderGlyph-grid cell, so the twin must give or_render_cell's bytes for every fixture glyph."""
import numpy as np
import pytest

import oracle_lib
import text_twin as tw
from font_renderer_amd.render_glyph import make_places, make_runs


@pytest.mark.parametrize("n,center,font_size", [(1, False, 24), (2, True, 17), (4, True, 40), (4, False, 11)])
def test_one_instance_is_the_oracle_cell(oracle, ascii_set, n, center, font_size):
    gs = ascii_set.gs
    checked = 0
    for g in range(len(ascii_set)):
        upm = int(ascii_set.g_upm[g])
        scale = np.float32(font_size) / np.float32(upm)
        c0, r0, w, h = tw.plain_cell(gs.boxes[g], scale, 0, 0)
        min_x, max_y = c0, -r0                                      # pen at the origin: column 0 is min_x, row 0 is max_y
        places = make_places([(g, -64 * min_x, max_y)])             # the cell at the run's (0, 0)
        runs = make_runs([(0, 1, w, h, 0, 0, scale)])
        got = tw.render_run("plain", gs, places, runs[0], n, center)
        want = oracle.render_cell(ascii_set.glyph(g), min_x, max_y, w, h, scale, oracle_lib.COVERAGE_U8, n, center)
        assert np.array_equal(got, want), (g, font_size, n, center)
        checked += 1
    assert checked == len(ascii_set)


def test_fractional_pen_shifts_the_samples(ascii_set):
    """pen_x64 + 64 is the same image one column to the right; fx != 0 adds the one column the shift can reach"""
    gs = ascii_set.gs
    g = ascii_set.find("Serif", "f")
    scale = np.float32(40) / np.float32(int(ascii_set.g_upm[g]))
    c0, r0, w, h = tw.plain_cell(gs.boxes[g], scale, 0, 0)
    base = tw.render_run("plain", gs, make_places([(g, -64 * c0 + 64 * 3, -r0)]), make_runs([(0, 1, w + 8, h, 0, 0, scale)])[0], 4, True)
    one = tw.render_run("plain", gs, make_places([(g, -64 * c0 + 64 * 4, -r0)]), make_runs([(0, 1, w + 8, h, 0, 0, scale)])[0], 4, True)
    assert np.array_equal(one[:, 1:], base[:, :-1]) and not one[:, 0].any()
    half = tw.render_run("plain", gs, make_places([(g, -64 * c0 + 64 * 3 + 32, -r0)]), make_runs([(0, 1, w + 8, h, 0, 0, scale)])[0], 4, True)
    assert not np.array_equal(half, base) and not np.array_equal(half, one)
    assert tw.plain_cell(gs.boxes[g], scale, 32, 0)[2] == w + 1

"""The instance matrix's case table (tests/instance_cases.py) against the instance set written from the template
parameter products: every kernel instance the dispatcher can launch has exactly one case, and every case has the
shape the GPU test (tests/test_gpu_instances.py) relies on.  No GPU, no library."""
import numpy as np

import fill_rule_ref as FR
import instance_cases as IC


def _glyph_arrays(gs, g):
    c0, c1 = int(gs.glyph_start[g]), int(gs.glyph_start[g + 1])
    p0 = int(gs.contour_start[c0])
    return gs.points_xy[p0:int(gs.contour_start[c1])], gs.contour_start[c0:c1 + 1] - np.uint32(p0)


def _row_crossings(case, job):
    """per sample row of the job: how many pieces of its glyph the row's ray crosses (the twin's exact rule)"""
    pts, cs = _glyph_arrays(case.gs, int(job["glyph"]))
    _, cy = FR.sample_axes(int(job["min_x"]), int(job["max_y"]), int(job["w"]), int(job["h"]), job["scale"], case.n, case.center)
    cyu, inv = np.unique(cy, return_inverse=True)
    cnt = np.zeros(len(cyu), np.int64)
    for (_, _, ylo, yhi, _) in FR.pieces(pts, cs):
        cnt += FR._crossed_rows(cyu, ylo, yhi)
    return cnt[inv], cy


def test_expected_set_is_the_246_instances():
    names = IC.expected_instances()
    assert len(names) == 246 and len(set(names)) == 246
    assert sum("cov4_kernel" in s for s in names) == 108
    assert sum("win1_kernel" in s for s in names) == 96
    assert sum("render_kernel" in s for s in names) == 42
    assert "fr::cov4_kernel<2, 8, 8, 2, 1>" in names and "fr::cov4_kernel<4, 32, 4, 4>" in names
    assert "fr::win1_kernel<3, 3, 16, 1>" in names and "fr::render_kernel<3, 4, 16, 3>" in names


def test_one_case_per_instance():
    """the predicted names over the table == the expected set: none missing, none twice, and each case predicts the
    instance it was built for"""
    cases = IC.build_cases()
    names = [IC.predicted_name(c) for c in cases]
    want = [s for s in IC.expected_instances() if s not in {u[0] for u in IC.UNREACHABLE}]
    assert sorted(names) == sorted(want)
    assert len(set(names)) == len(names) == 246 - len(IC.UNREACHABLE)
    for c, name in zip(cases, names):
        k = c.key
        tail = ", 1>" if k[-1] else ">"
        built_for = {"cov4": "fr::cov4_kernel<{1}, {2}, {3}, {4}", "win1": "fr::win1_kernel<{1}, {2}, {3}",
                     "render": "fr::render_kernel<{1}, {2}, {3}, {4}"}[c.family].format(*k) + tail
        assert name == built_for


def test_unreachable_list():
    """instances proven unreachable through the public API, each with the line of the C ABI units (csrc/fr_api_*.hip) that proves it: none"""
    assert IC.UNREACHABLE == []


def test_cases_are_single_class_plans():
    """2-3 jobs, all of one predicted class (merge_small_classes leaves a plan's only class alone), on the expected side
    of the fast / general split"""
    for c in IC.build_cases():
        cl = IC.job_classes(c)
        assert 2 <= len(cl) <= 3 and len(set(cl)) == 1, (c.key, cl)
        assert (cl[0] == 0) == (c.family == "render"), (c.key, cl)
        assert len(c.gs) == len(c.jobs) and sorted(int(g) for g in c.jobs["glyph"]) == list(range(len(c.jobs)))


def test_cell_shapes():
    """ragged strips (61 / 125 / 261 pixels: WLOG 2 / 3 / 4, the last with a second strip of 5), five wave bands with a
    ragged last one, odd out_x, a stride that is no multiple of 16, sentinels on every side; the two uniform
    render_kernel instances on uniform cells"""
    for c in IC.build_cases():
        H, S = c.shape
        assert S % 16 != 0
        band = 16 if c.n != 2 else 32
        uniform = c.family == "render" and c.key[4] > 0
        for j in c.jobs:
            w, h, ox, oy = (int(j[f]) for f in ("w", "h", "out_x", "out_y"))
            assert ox % 2 == 1 and ox >= 1 and oy >= 1 and ox + w < S and oy + h < H
            if uniform:
                assert (w, h) == ({4: 256, 3: 128}[c.key[4]], 64)
            else:
                assert w in (61, 125, 261) and h == 4 * band + 5
            if c.family != "render":
                assert w == IC.WIDTHS[c.key[1]]
        # the cells do not touch: at least one sentinel column between neighbours
        xs = sorted((int(j["out_x"]), int(j["w"])) for j in c.jobs)
        assert all(a[0] + a[1] < b[0] for a, b in zip(xs, xs[1:]))


def test_both_sample_phases_in_every_group():
    seen = {}
    for c in IC.build_cases():
        seen.setdefault(IC.group_of(c), set()).add(bool(c.center))
    assert sorted(seen, key=str) == sorted(IC.groups(), key=str)
    assert all(v == {False, True} for v in seen.values()), seen


def test_crossing_counts_either_side_of_cap():
    """across a case's jobs some sample row's ray meets exactly CAP crossings and one meets CAP + 2 (counted with the
    fill-rule twin's pieces); the RPL-2 / CAP-16 class holds <= 16 crossings per ray, so the exactly-CAP row only;
    win1_kernel: 16 and 34 (the RPL-2 class: 16).  The comb that carries them lies inside the cell's first strip."""
    for c in IC.build_cases():
        counts = set()
        for j in c.jobs[1:]:
            cnt, cy = _row_crossings(c, j)
            counts |= set(int(v) for v in cnt)
            pts, _ = _glyph_arrays(c.gs, int(j["glyph"]))
            s = float(j["scale"])
            comb = pts[pts[:, 1] <= IC.COMB_ROWS[1]]
            assert comb[:, 0].min() * s >= int(j["min_x"]) and comb[:, 0].max() * s < int(j["min_x"]) + min(int(j["w"]), 16 << c_wlog(c))
            assert ((cy >= IC.COMB_ROWS[0]) & (cy < IC.COMB_ROWS[1])).sum() >= 2 * c.n        # rows through the teeth
        if c.family == "win1":
            want = {16} if c.key[3] == 2 else {16, 34}
        else:
            cap = c.key[2] if c.family == "cov4" else c.key[3]
            want = {cap} if (c.family == "cov4" and c.key[3] == 2 and cap == 16) else {cap, cap + 2}
        assert want <= counts, (c.key, sorted(counts))
        if c.family != "render" and c.key[3] == 2:
            assert max(counts) <= 16, (c.key, sorted(counts))


def c_wlog(c):
    """the strip width class of a case's cells"""
    w = int(c.jobs["w"][0])
    return 2 if w <= 64 else (3 if w <= 128 else 4)


def test_predictor_rules_on_hand_made_glyphs():
    """the restated bounds on shapes whose counts are known: a comb of T teeth has 4 T + 2 segments, root bound 2 T + 1
    and ray bound 2 T; the ballast comb adds its own above it without touching the comb's rows"""
    from font_renderer_amd.glyph import GlyphSet
    for T in (4, 8, 17):
        gs = GlyphSet([IC.comb_ballast_glyph(T, 0)])
        s = IC.glyph_segments(gs, 0)
        assert (len(s), IC.root_bound(s), IC.ray_bound(s)) == (4 * T + 2, 2 * T + 1, 2 * T)
    gs = GlyphSet([IC.comb_ballast_glyph(8, 70)])
    s = IC.glyph_segments(gs, 0)
    assert (len(s), IC.root_bound(s), IC.ray_bound(s)) == (34 + 282, 17 + 141, 140)
    # one quadratic whose control point overshoots both ends: two candidate roots, met twice above the ends
    arc = np.array([[[0, 0], [50, 100], [100, 0]]], np.int64)
    assert IC.root_bound(arc) == 2 and IC.ray_bound(arc) == 2
    flat = np.array([[[0, 5], [50, 5], [100, 5]]], np.int64)
    assert IC.root_bound(flat) == 0
    assert IC.fast_class(4, 64, 512, 10, 10, 2) == 1 and IC.fast_class(4, 64, 513, 10, 10, 2) == 0
    assert IC.fast_class(1, 129, 10, 769, 10, 2) == 0 and IC.fast_class(1, 129, 10, 768, 1024, 2) == 12
    assert IC.fast_class(2, 65, 10, 256, 128, 17) == 6 and IC.fast_class(2, 65, 10, 257, 128, 2) == 7

"""Every raster kernel instance the dispatcher can launch, by name: 246 tiny single-class plans (tests/instance_cases.py,
checked on the CPU by tests/test_instance_cases.py), one per instance of cov4_kernel, win1_kernel and render_kernel.

Per case: the plan's first kernel, as fr_plan_describe prints it, is exactly the predicted instance with every job on
it; then the plan is rendered into a sentinel-filled array three times — with the defaults (the cell's wave bands split
over two workgroups), with min_wgs = 1 (one workgroup walks all five bands) and with fuse_prepare = 0 (records prepared
stand-alone) — and each render equals the CPU reference over the WHOLE array, sentinels included.  The reference is the C
oracle for flags = 0 and the numpy twin of FR_FILL_CONSISTENT (tests/fill_rule_ref.py, every row) for FILL = 1.  Byte
equality throughout; the one leniency is the SDF under FILL = 1 on the pixels where the two fill rules disagree."""
import numpy as np
import pytest

import fill_rule_ref as FR
import font_renderer_amd as fr
import instance_cases as IC
import oracle_lib as O
from font_renderer_amd import render_glyph as rg

pytestmark = pytest.mark.gpu
DEFAULTS = {"kmax": 32, "cov4": 1, "min_wgs": 2048, "fuse_prepare": 1}
VARIANTS = (("defaults", {}), ("min_wgs=1", {"min_wgs": 1}), ("fuse_prepare=0", {"fuse_prepare": 0}))
# one test per (family, NS or MODE, FILL) and, for the fast kernels, strip width: a few seconds of CPU reference each
CASES = {}
for _c in IC.build_cases():
    CASES.setdefault(IC.group_of(_c) + ((_c.key[1],) if _c.family != "render" else ()), []).append(_c)

_twin_windings = {}        # FILL = 1: sample windings per job geometry, shared by the modes that render the same cells


def _blank(case):
    return np.full(case.shape, IC.SENTINEL, np.int16 if case.mode == IC.WINDING_I16 else np.uint8)


def _oracle(oracle, case, mode):
    out = np.full(case.shape, IC.SENTINEL, np.int16 if mode == IC.WINDING_I16 else np.uint8)
    return oracle.render_batch(case.gs, case.jobs, mode, out, case.n, case.center, 16)


def _twin(case, mode):
    """FR.render_batch with the sample windings of a job kept for the next mode over the same cell"""
    out = np.full(case.shape, IC.SENTINEL, np.int16 if mode == IC.WINDING_I16 else np.uint8)
    gs = case.gs
    for j in case.jobs:
        g = int(j["glyph"])
        c0, c1 = int(gs.glyph_start[g]), int(gs.glyph_start[g + 1])
        p0 = int(gs.contour_start[c0])
        pts, cs = gs.points_xy[p0:int(gs.contour_start[c1])], gs.contour_start[c0:c1 + 1] - np.uint32(p0)
        geom = tuple(int(j[f]) for f in ("min_x", "max_y", "w", "h")) + (float(j["scale"]), case.n, bool(case.center))
        key = (pts.tobytes(), cs.tobytes(), geom)
        if key not in _twin_windings:
            cx, cy = FR.sample_axes(*geom[:4], j["scale"], case.n, case.center)
            wd = FR.winding_fill(pts, cs, cx[None, :], cy[:, None])
            wd.setflags(write=False)
            _twin_windings[key] = wd
        img = FR.to_mode(_twin_windings[key], mode, case.n)
        oy, ox = int(j["out_y"]), int(j["out_x"])
        out[oy:oy + img.shape[0], ox:ox + img.shape[1]] = img
    return out


def _check(case, got, ref, what):
    bad = np.argwhere(got != ref)
    assert bad.size == 0, (what, len(bad), "first (row, col):", bad[:4].tolist(),
                           "got", [int(got[tuple(b)]) for b in bad[:4]], "want", [int(ref[tuple(b)]) for b in bad[:4]])


@pytest.mark.parametrize("group", list(CASES), ids=lambda g: "-".join(str(v) for v in g[:2]) + f"-fill{g[2]}" + (f"-wlog{g[3]}" if len(g) > 3 else ""))
def test_every_instance_of_the_group(ctx, oracle, group):
    """all (record class, CAP) instances of one (family, NS or MODE, FILL, WLOG) — render_kernel: all (CAP, WLOG) of one
    (MODE.N, FILL): name, job split and three renders each"""
    cases = CASES[group]
    assert len(cases) == {"cov4": 9, "win1": 4}.get(group[0], 9 if group[1] == "3.4" else 3)
    sdf_moved = 0
    try:
        for case in cases:
            name = IC.predicted_name(case)
            flags = fr.FR_FILL_CONSISTENT if case.fill else 0
            phase = fr.FR_SAMPLE_CENTER if case.center else fr.FR_SAMPLE_CORNER
            ctx.set_option("kmax", case.kmax)
            ctx.set_option("cov4", 0 if case.family == "render" else 1)
            dgs = fr.DeviceGlyphSet(ctx, case.gs)
            try:
                plan = fr.Plan(dgs, case.jobs, case.mode, case.n, phase, flags)
                st, desc = plan.stats(), plan.describe()
                plan.close()
                assert desc.split("; ")[0] == f"{name} x{len(case.jobs)}", (case.key, desc)
                fast = 0 if case.family == "render" else len(case.jobs)
                assert st == {"jobs_cov4": fast, "jobs_general": len(case.jobs) - fast}, (case.key, st, desc)
                # the CPU reference, once per case
                same = None
                if case.mode != IC.SDF_U8:
                    ref = _twin(case, case.mode) if case.fill else _oracle(oracle, case, case.mode)
                else:
                    ref = _oracle(oracle, case, O.SDF_U8)
                    if case.fill:
                        mask = _twin(case, IC.MASK_NONZERO)
                        same = mask == _oracle(oracle, case, O.MASK_NONZERO)
                        sdf_moved += int((~same).sum())
                assert (ref != IC.SENTINEL).any()
                for what, opts in VARIANTS:
                    for k, v in opts.items():
                        ctx.set_option(k, v)
                    got = rg.render_batch(dgs, case.jobs, case.mode, _blank(case), case.n, phase, flags)
                    for k in opts:
                        ctx.set_option(k, DEFAULTS[k])
                    if same is None:
                        _check(case, got, ref, (name, what))
                    else:
                        # where both rules fill alike: the oracle's byte; elsewhere: the twin's side of 128, or 128
                        _check(case, np.where(same, got, 0), np.where(same, ref, 0), (name, what))
                        wrong = ~same & (((mask == 255) & (got < 128)) | ((mask == 0) & (got > 128)))
                        assert not wrong.any(), (name, what, np.argwhere(wrong)[:4].tolist())
            finally:
                dgs.close()
    finally:
        for k, v in DEFAULTS.items():
            ctx.set_option(k, v)
    if group[0] == "win1" and group[1] == 3 and group[2] == 1:
        assert sdf_moved > 0          # some case has pixels that the two fill rules sign differently

"""The host arithmetic of the C ABI (csrc/fr_host_rules.cpp) on the CPU: host/host_rules_selftest runs both atlas layouts,
fr_render_glyph_dims, the sRGB conversions, fr_rgba_unpremultiply, the four argument checks and fr_render_glyph's arena
layout and prints one line per case.  tests/golden/host_rules.json holds those lines as tools/mint_host_rules.py made
them through ctypes from the library as it was while this arithmetic still lived in the HIP unit of the C ABI; the
lines of what that library could not answer without a device (check_params, check_flags, check_job, the arena) are
restated here on their own."""
import json
import os
import re

import host_selftest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "host_rules.json")


def _lines():
    return host_selftest.named("host_rules_selftest")


def test_host_rules_match_golden():
    got = _lines()
    with open(GOLDEN) as f:
        want = json.load(f)
    assert list(got) == list(want), "the cases differ from the golden file's"
    wrong = {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    assert not wrong, wrong


def test_every_limit_is_met_on_both_sides():
    """a case named -max / -min / -last / -in sits on a limit and passes; its -over / -under / -out twin lies one step
    beyond and is refused with FR_E_INVALID or FR_E_UNSUPPORTED"""
    inside, outside = 0, 0
    for name, text in _lines().items():
        rc = int(re.match(r"rc=(-?\d+)", text).group(1))
        if re.search(r"-(max|min|last|in)$", name):
            assert rc == 0, (name, text)
            inside += 1
        elif re.search(r"-(over|under|out)$", name):
            assert rc in (-1, -4) and "err=" in text, (name, text)
            outside += 1
    assert inside >= 15 and outside >= 15, (inside, outside)


def test_check_params_restated():
    """check_params: mode in 0..4; n in {1, 2, 4} for coverage (else FR_E_UNSUPPORTED) and 1 otherwise (else FR_E_INVALID);
    then the phase in {0, 1}"""
    cases = {k: v for k, v in _lines().items() if k.startswith("check_params/mode")}
    assert len(cases) == 42 + 6
    for name, text in cases.items():
        mode, n, phase = (int(v) for v in re.match(r"check_params/mode(-?\d+)-n(\d+)-phase(-?\d+)", name).groups())
        if not 0 <= mode <= 4:
            want = -1
        elif mode == 3:
            want = 0 if n in (1, 2, 4) else -4
        else:
            want = 0 if n == 1 else -1
        if want == 0 and phase not in (0, 1):
            want = -1
        assert text.startswith("rc=%d " % want), (name, text)


def test_arena_layout_restated():
    """glyph_arena: every part at the next multiple of 16 behind the one before it, in the order and with the paddings
    fr_render_glyph has always used"""
    cases = {k: v for k, v in _lines().items() if k.startswith("arena/")}
    assert len(cases) >= 6
    al = lambda v: (v + 15) & ~15
    for name, text in cases.items():
        np_, ns, rec, img = (int(v) for v in re.match(r"arena/np(\d+)-ns(\d+)-rec(\d+)-img(\d+)", name).groups())
        got = {k: int(v) for k, v in (f.split("=") for f in text.split(" ")[1:])}
        want = {"pts": 0}
        want["p0"] = al(np_ * 4 + 16)
        want["spts"] = al(want["p0"] + ns * 4 + 4)
        want["gseg"] = al(want["spts"] + ns * 12 + 16)
        want["job"] = al(want["gseg"] + 8)
        want["jseg"] = al(want["job"] + 32)
        want["large"] = al(want["jseg"] + 8)
        want["up"] = want["cnt"] = al(want["large"] + 4)
        want["recs"] = al(want["cnt"] + 8)
        want["out"] = al(want["recs"] + max(ns, 1) * 2 * rec)
        want["total"] = al(want["out"] + img)
        assert got == want, name

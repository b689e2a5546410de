"""The launches of a text plan's render (text_launches and text_launch_name, csrc/fr_text_plan.cpp) on the CPU:
host/text_plan_selftest launches prints the launch list of a handful of plans — a cached one, an FR_TEXT_LOAD plan whose
placements are all clipped away, plans with tiles and no instance — and the kernel name of every key in a box around
the valid ones.  tests/golden/text_launches.json holds the list lines; each was compared with the fr_plan_describe strings
the GPU tests pin for the same kind of plan.  tests/golden/text_kernel_names.json holds the function symbols of the three
text units' device code as they stood before the launch list carried the instance, demangled, without "void " and the
argument list: the names rocprofv3 shows."""
import json
import os

import host_selftest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def _lines():
    return host_selftest.named("text_plan_selftest", "launches")


def _golden(name):
    with open(os.path.join(GOLDEN, name)) as f:
        return json.load(f)


def test_the_launch_lists_match_golden():
    got = {k: v for k, v in _lines().items() if not k.startswith("name/")}
    want = _golden("text_launches.json")
    assert list(got) == list(want), "the cases differ from the golden file's"
    wrong = {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    assert not wrong, wrong
    # the short lists the render and the description must agree on
    assert got["load_all_clipped_away/plain/launches"] == "0" and got["no_runs/affine/launches"] == "0"
    assert got["tiles_but_no_instance/affine/launch0"] == "text fr::text_affine_kernel<4, 0> grid 2 count 0"
    assert [got[f"coverage_cached/plain/launch{i}"].split(" ")[0] for i in range(3)] == ["prepare", "mask", "cached"]


def test_the_named_keys_are_exactly_the_kernels():
    """three forms x (3 N x 2 FILL coverage + 4 colour families x 3 N x 2 FILL x 3 BLEND) = 234 text kernels, 3 + 4 x 3 x 3
    = 39 composites, 3 x 2 mask kernels: every one of the 279 device functions is named by exactly one key, and the other
    keys of the box (a fourth form, colour families -1 and 5, N in {0, 3, 5}, FILL -1 and 2, BLEND -1 and 3, coverage with
    BLEND != 0) get no name"""
    lines = _lines()
    named = [v for k, v in lines.items() if k.startswith("name/") and k != "name/swept"]
    want = _golden("text_kernel_names.json")
    assert len(want) == len(set(want)) == 279 == 3 * (3 * 2 + 4 * 3 * 2 * 3) + (3 + 4 * 3 * 3) + 3 * 2
    assert len(named) == len(set(named)), "two keys share a name"
    assert set(named) == set(want), (sorted(set(want) - set(named)), sorted(set(named) - set(want)))
    assert lines["name/swept"] == "keys 3594 named 279"

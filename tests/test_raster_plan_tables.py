"""The host rules of raster plans (csrc/fr_raster_plan.cpp) on the CPU: host/raster_plan_selftest runs fast_rule,
fast_class, merge_small_classes, split_bands, the plan builder with its launch list, the single-glyph call's use of it
and the two glyph bounds on synthetic number tables and prints one line per case.
tests/golden/raster_plan_tables.json holds those lines as minted from the rules' text as it stood in fr_api.hip, moved
but not yet restructured; its name/ lines (the kernel instance of every launch, raster_launch_name) were minted when the
launch list began to carry the instance."""
import json
import os

import numpy as np

import host_selftest
import instance_cases as ic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "raster_plan_tables.json")


def _lines():
    return host_selftest.named("raster_plan_selftest")


def test_raster_plan_tables_match_golden():
    got = _lines()
    with open(GOLDEN) as f:
        want = json.load(f)
    assert list(got) == list(want), "the cases differ from the golden file's"
    wrong = {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    assert not wrong, wrong


def test_bounds_match_the_python_restatement():
    """glyph_root_bound and glyph_ray_bound against root_bound and ray_bound of instance_cases.py, written independently"""
    cases = {k: v for k, v in _lines().items() if k.startswith("bounds/")}
    assert len(cases) >= 8
    for name, text in cases.items():
        fields = dict(f.split("=") for f in text.split(" "))
        segs = np.array([int(v) for v in fields["segs"].split(",") if v], np.int64).reshape(-1, 3, 2)
        assert (int(fields["root"]), int(fields["ray"])) == (ic.root_bound(segs), ic.ray_bound(segs)), name


def test_the_rules_name_exactly_the_expected_instances():
    """the name/sweep/ lines — every value the rules can give each template argument, both fill rules — against
    expected_instances of instance_cases.py, written from the template parameter products: none missing, none extra"""
    named = [n for k, v in _lines().items() if k.startswith("name/sweep/") for n in v.split("; ") if n]
    want = ic.expected_instances()
    assert len(want) == len(set(want)) == 246
    assert len(named) == len(set(named)), "a sweep line names an instance twice"
    assert set(named) == set(want), (sorted(set(want) - set(named)), sorted(set(named) - set(want)))

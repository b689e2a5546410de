"""The host tables of text plans (csrc/fr_text_plan.cpp) on the CPU: host/text_plan_selftest runs the builder on a fixed
list of small cases in all three placement forms, checks by brute force what the kernels rely on (cells inside their
runs, exact tile lists in placement order, no empty tile under FR_TEXT_LOAD, exact glyph list) and prints one FNV-1a
hash over every returned vector and scalar per case, or the error code and message of a failing case.
tests/golden/text_plan_tables.json holds those lines as minted from the builder's text before it was restructured."""
import json
import os
import re

import host_selftest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "text_plan_tables.json")


def test_text_plan_tables_match_golden():
    got = host_selftest.named("text_plan_selftest")
    with open(GOLDEN) as f:
        want = json.load(f)
    assert list(got) == list(want), "the cases differ from the golden file's"
    wrong = {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    assert not wrong, wrong
    # every message of the builder but the one that needs 2^32 tile / instance pairs has a failing case
    texts = {re.sub(r"\d+", "#", v.split(": ", 1)[1]) for v in want.values() if v.startswith("error ")}
    assert len(texts) == 20, sorted(texts)

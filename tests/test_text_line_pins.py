"""The line builders of font_renderer_amd.text against tests/golden/text_line_pins.json: every entry is recomputed by
tests/golden/make_text_line_pins.py, one font and size at a time, and compared.  Host arithmetic only: no device."""
import json
import os
import sys

import pytest

from fixtures import GOLDEN

sys.path.insert(0, GOLDEN)
import make_text_line_pins as M  # noqa: E402

with open(os.path.join(GOLDEN, "text_line_pins.json")) as f:
    PINS = json.load(f)


def _pinned(group):
    return {k: v for k, v in PINS.items() if k.startswith(f"{group[0]}/{group[1]}/")}


def test_groups_partition_the_file():
    """every pinned entry belongs to exactly one group, and the cases that draw nothing are pinned as such"""
    per_string = len(M.SLANTS) + 1 + len(M.VIEWS) + 2 * len(M.ANGLES) + 1
    assert sum(len(_pinned(g)) for g in M.GROUPS) == len(PINS) == len(M.GROUPS) * len(M.STRINGS) * per_string
    nothing = [k for k, v in PINS.items() if v is None]
    assert len(nothing) == len(M.GROUPS) * (len(M.SLANTS) + 1) and all("/spaces/" in k for k in nothing)


@pytest.mark.parametrize("group", M.GROUPS, ids=[f"{n}-{s}" for n, s in M.GROUPS])
def test_line_builders_are_pinned(group):
    got, want = M.compute(group), _pinned(group)
    assert sorted(got) == sorted(want)
    for key in want:
        assert got[key] == want[key], key

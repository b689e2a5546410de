"""The CPU twins of the text path against tests/golden/text_twin_hashes.json: every entry is recomputed by
tests/golden/make_text_twin_hashes.py, group by group, and compared, so a change to a twin is seen on its own output."""
import json
import os
import sys

import pytest

from fixtures import GOLDEN

sys.path.insert(0, GOLDEN)
import make_text_twin_hashes as M  # noqa: E402

with open(os.path.join(GOLDEN, "text_twin_hashes.json")) as f:
    PINS = json.load(f)


def _prefix(group):
    """the keys of a group start with this"""
    if group[0] != "rgba":
        return "/".join(group)
    _, form, n, srgb, load = group
    return f"rgba/{form}/n{n}/{'srgb' if srgb else 'unorm'}/{'load' if load else 'clear'}"


def _pinned(group):
    return {k: v for k, v in PINS.items() if k == _prefix(group) or k.startswith(_prefix(group) + "/")}


def test_groups_partition_the_file():
    """every pinned entry belongs to exactly one group, so the parametrised test below leaves none unchecked"""
    assert len(set(M.GROUPS)) == len(M.GROUPS)
    assert sum(len(_pinned(g)) for g in M.GROUPS) == len(PINS) == 13 + 10 + 2 + 144
    assert all(_pinned(g) for g in M.GROUPS)


@pytest.mark.parametrize("group", M.GROUPS, ids=["-".join(str(v) for v in g) for g in M.GROUPS])
def test_twin_output_is_pinned(group):
    got, want = M.compute(group), _pinned(group)
    assert sorted(got) == sorted(want)
    for key in want:
        assert got[key] == want[key], key

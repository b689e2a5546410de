"""Every text kernel instance a plan can launch, by name and by bytes: one tiny plan per key of tests/text_instance_cases.py
(234 of the three placement forms, 39 FR_TEXT_CACHE composites that between them reach the six mask kernels).

Per key: fr_plan_describe's whole string equals the one built from the key, with every kernel name a member of
tests/golden/text_kernel_names.json (the function symbols of the text units' device code); and the SHA-256 of the whole
output buffer, border included, equals tests/golden/text_instance_hashes.json.  Those hashes were recorded from the
library as it stood before the launch list carried the instance (FR_TEXT_INSTANCE_MINT=<file> records instead of
comparing), so they pin what each instance computed then; the fixture's own conditions — a cached key renders its plain
twin's bytes, and otherwise no two keys of one output format render the same bytes unless the fixture says why — make a
wrong look-up fail."""
import hashlib
import json
import os
from contextlib import closing

import numpy as np
import pytest

import font_renderer_amd as fr
import text_gpu as G
import text_instance_cases as T

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MINT = os.environ.get("FR_TEXT_INSTANCE_MINT")
GROUPS = {"plain": [k for k in T.plain_keys() if k.form == 0], "place": [k for k in T.plain_keys() if k.form == 1],
          "affine": [k for k in T.plain_keys() if k.form == 2], "cached": T.cached_keys()}


def _golden(name):
    with open(os.path.join(GOLDEN, name)) as f:
        return json.load(f)


def _describe_and_hash(ctx, dgs, k):
    """the key's plan over its start buffer -> (describe, SHA-256 of the whole buffer)"""
    places, runs, flags = T.places_of(k.form), T.runs(), T.flags_of(k)
    start = T.start_buffer(k)
    info = {}
    if k.fam == 0:
        got = G.render_gray(ctx, dgs, places, runs, T.SHAPE, fr.FR_COVERAGE_U8, k.n, False, flags, sent=T.SENT, info=info)
    else:
        cols = T.TRANSLUCENT if k.blend else T.OPAQUE
        got = G.render_rgba(ctx, dgs, places, cols, runs, None if k.fam in (3, 4) else T.CLEAR, start, k.n, False, flags, info=info)
    border = np.ones(T.SHAPE, bool)
    border[T.RUN[5]:T.RUN[5] + T.RUN[3], T.RUN[4]:T.RUN[4] + T.RUN[2]] = False
    assert np.array_equal(got[border], start[border]), (T.key_id(k), "a byte outside the run changed")
    assert not np.array_equal(got, start), T.key_id(k)
    return info["describe"], hashlib.sha256(got.tobytes()).hexdigest()


def _record(got):
    """adds a group's hashes to the file MINT and lists the plain keys of one output format that share one"""
    fixture = {"sha256": {}}
    if os.path.exists(MINT):
        with open(MINT) as f:
            fixture = json.load(f)
    sha = fixture["sha256"]
    sha.update(got)
    plain = [k for k in T.plain_keys() if T.key_id(k) in sha]
    fixture["same_bytes"] = [{"keys": [T.key_id(a), T.key_id(b)], "reason": T.same_bytes_reason(a, b)}
                             for i, a in enumerate(plain) for b in plain[i + 1:]
                             if (a.fam == 0) == (b.fam == 0) and sha[T.key_id(a)] == sha[T.key_id(b)]]
    with open(MINT, "w") as f:
        json.dump(fixture, f, indent=0, sort_keys=True)
        f.write("\n")


@pytest.mark.gpu
@pytest.mark.parametrize("group", list(GROUPS))
def test_every_instance_of_the_group(ctx, ascii_set, group):
    names = set(_golden("text_kernel_names.json"))
    want = {} if MINT else _golden("text_instance_hashes.json")["sha256"]
    got = {}
    with closing(fr.DeviceGlyphSet(ctx, T.glyph_set(ascii_set))) as dgs:
        for k in GROUPS[group]:
            assert T.kernel_name(k) in names and (not k.cached or T.mask_name(k) in names), T.key_id(k)
            desc, sha = _describe_and_hash(ctx, dgs, k)
            assert desc == T.describe_of(k), (T.key_id(k), desc)
            got[T.key_id(k)] = sha
    if MINT:
        _record(got)
        return
    wrong = [i for i in got if got[i] != want.get(i)]
    assert not wrong, wrong


def test_the_fixture_tells_the_instances_apart():
    """the conditions on text_instance_hashes.json: every key has a hash, a cached key's is its plain twin's, and two plain
    keys of one output format share a hash only where the fixture lists the pair with the reason the cases module gives"""
    fixture = _golden("text_instance_hashes.json")
    sha = fixture["sha256"]
    keys = T.plain_keys() + T.cached_keys()
    assert len(T.plain_keys()) == 234 and len(T.cached_keys()) == 39 and sorted(sha) == sorted(T.key_id(k) for k in keys)
    assert {(k.n, k.fill) for k in T.cached_keys()} == {(n, f) for n in (1, 2, 4) for f in (0, 1)}
    assert {T.kernel_name(k) for k in keys} | {T.mask_name(k) for k in T.cached_keys()} == set(_golden("text_kernel_names.json"))
    for k in T.cached_keys():
        assert sha[T.key_id(k)] == sha[T.key_id(T.twin_of(k))], T.key_id(k)
    listed = {tuple(p["keys"]): p["reason"] for p in fixture["same_bytes"]}
    plain = T.plain_keys()
    found = {}
    for i, a in enumerate(plain):
        for b in plain[i + 1:]:
            if (a.fam == 0) == (b.fam == 0) and sha[T.key_id(a)] == sha[T.key_id(b)]:
                found[(T.key_id(a), T.key_id(b))] = T.same_bytes_reason(a, b)
    assert found == listed and all(found.values()), sorted(set(found.items()) ^ set(listed.items()))

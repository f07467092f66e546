"""CPU-only: every argument check of csrc/abi.hip answers with the return code and the crnerf_last_error() text recorded in
tests/golden/abi_errors.json (tools/make_abi_error_golden.py: the cases, and how the fixture was recorded).  The text is part of the contract:
callers match on it."""
import json
import os
import sys

import pytest

from crnerf_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_abi_error_golden as G  # noqa: E402


@pytest.fixture(scope="module")
def table():
    with open(G.GOLDEN) as f:
        return json.load(f)


def test_fixture_holds_every_case_and_none_that_reached_a_launch(table):
    assert sorted(table) == sorted(G.key(e, label) for e, label, _, _ in G.CASES)
    assert len(table) == len(G.CASES)                                   # no two cases share a name
    assert G.fixture_faults(table) == []
    assert {e for e, _, _, _ in G.CASES} <= set(_lib.ALL_SIGNATURES)
    assert sum(is_noop for _, _, _, is_noop in G.CASES) >= 40 and all(table[G.key(e, label)]["message"] == G.PRIME[1]
                                                                      for e, label, _, is_noop in G.CASES if is_noop)


def test_every_refused_call_answers_as_recorded(table):
    # a fixture with a case that got through validation when it was recorded must not be replayed: on a GPU it launches on the dummy pointers
    assert G.fixture_faults(table) == [] and sorted(table) == sorted(G.key(e, label) for e, label, _, _ in G.CASES)
    lib = _lib.load()
    wrong = []
    for e, label, mut, is_noop in G.CASES:
        want = table[G.key(e, label)]
        got = G.run_case(lib, _lib, e, mut, is_noop)
        if got != (want["code"], want["message"]):
            wrong.append("%s: %r, recorded %r" % (G.key(e, label), got, (want["code"], want["message"])))
    assert not wrong, "%d of %d cases:\n%s" % (len(wrong), len(G.CASES), "\n".join(wrong[:20]))

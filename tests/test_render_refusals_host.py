"""CPU-only: every refusal of ops.render_rays, ops.render_coarse_weights and ops.render_rays_bf16_fine that fires before a device tensor is needed
answers with the exception type and the full message recorded in tests/golden/render_refusals.json (tools/make_render_refusal_golden.py: the cases,
and how the fixture was recorded).  Which rule answers when a call breaks two is part of what is recorded."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_render_refusal_golden as G  # noqa: E402


@pytest.fixture(scope="module")
def table():
    with open(G.GOLDEN) as f:
        return json.load(f)


def test_fixture_holds_every_case(table):
    names = [name for name, _, _, _ in G.cases()]
    assert len(set(names)) == len(names) and sorted(table) == sorted(names)
    assert {name.split(" / ")[0] for name in names} == {"render_rays", "render_coarse_weights", "render_rays_bf16_fine"}
    assert {t for t, _ in table.values()} == {"ValueError", "RuntimeError"}


def test_every_refused_call_answers_as_recorded(table):
    wrong = []
    for name, fn, args, kw in G.cases():
        got = G.run_case(fn, args, kw)
        if got != table[name]:
            wrong.append("%s: %r, recorded %r" % (name, got, table[name]))
    assert not wrong, "%d cases:\n%s" % (len(wrong), "\n".join(wrong[:20]))

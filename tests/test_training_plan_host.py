"""The training settings of crnerf_amd.autograd against tests/golden/training_plan.json (tools/make_training_plan_golden.py: recorded while every
getter read the environment itself): the getters and training_plan() answer every recorded row alike, and the environment is read at call time.
No GPU needed."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_training_plan_golden as G  # noqa: E402

from crnerf_amd import autograd as AG  # noqa: E402


@pytest.fixture(scope="module")
def table():
    with open(G.GOLDEN) as f:
        return json.load(f)


def test_the_rows_are_the_recorded_rows(table):
    assert sorted(G.row_name(r) for r in G.rows()) == sorted(table) and len(table) >= 200


def test_the_getters_give_the_recorded_rows(table):
    for r in G.rows():
        with G.applied(r):
            got = G.getter_answers()
        want = table[G.row_name(r)]
        assert got == want and [type(g) for g in got] == [type(w) for w in want], (r, got, want)


def test_training_plan_gives_the_recorded_rows(table):
    for r in G.rows():
        with G.applied(r):
            p = AG.training_plan()
            got = [p.forward, p.family == "bf16", p.wgrad_code(False), p.wgrad_code(True), p.recompute, p.bf16_fused, p.chunk_points]
        want = table[G.row_name(r)]
        assert got == want and [type(g) for g in got] == [type(w) for w in want], (r, got, want)
        assert p.family in ("f32", "bf16")


def test_training_plan_reads_the_environment_at_call_time(monkeypatch):
    for k in G.VARIABLES:
        monkeypatch.delenv(k, raising=False)
    a = AG.training_plan()
    monkeypatch.setenv("CRNERF_TRAIN_CHUNK_POINTS", "212")
    monkeypatch.setenv("CRNERF_TRAIN_FWD", "x3")
    b = AG.training_plan()
    assert (a.chunk_points, a.forward) == (1 << 21, "auto") and (b.chunk_points, b.forward) == (212, "f32x3")
    with pytest.raises(AttributeError):
        b.forward = "f32"                                # a plan is immutable: forward and backward of a render read the same one
    monkeypatch.delenv("CRNERF_TRAIN_FWD")
    assert AG.training_plan().forward == "auto" and AG.get_training_forward_mode() == "auto"

"""Every training mode of the render node against tests/golden/g_train_render_parent.json (tools/make_train_render_golden.py, which owns the cases
and their inputs): the SHA-256 of the six outputs and the 48 parameter gradients of a grad-mode render, recorded while autograd.py had one node
class per mode and every getter read the environment itself.  One TrainPlan per render call and one node for all modes must give the same bytes."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("make_train_render_golden", os.path.join(ROOT, "tools", "make_train_render_golden.py"))
G = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(G)


@pytest.fixture(scope="module")
def table():
    with open(G.GOLDEN) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def inputs():
    return G.Inputs()


def test_every_case_is_recorded(table):
    assert sorted(table) == sorted(G.case_name(c) for c in G.CASES)


@pytest.mark.parametrize("case", G.CASES, ids=[G.case_name(c) for c in G.CASES])
def test_outputs_and_gradients_are_the_recorded_bytes(case, table, inputs):
    want = table[G.case_name(case)]
    got = G.digests(inputs, case)
    assert sorted(got) == sorted(want)
    if case[0] == "fine_only":
        assert all(got[k] is None for k in got if k.startswith("grad/coarse."))
    wrong = []
    for k in sorted(want):
        if got[k] != want[k]:
            wrong.append(k)
            print("%s: %s differs: %s, recorded %s" % (G.case_name(case), k, "None" if got[k] is None else "shape %s max|.| %r" % tuple(got[k][1:]),
                                                     "None" if want[k] is None else "shape %s max|.| %r" % tuple(want[k][1:])))
    assert not wrong, wrong

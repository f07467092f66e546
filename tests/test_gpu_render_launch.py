"""The launch layer between csrc/abi.hip and the kernels (csrc/launch.h and the render / MLP launchers on top of it) decides nothing about what is
computed: it checks, fills the kernel's parameter block, plans the grid and launches.  So every output of every kernel variant must equal, bit for
bit, what the build before launch.h returned -- with every optional field of the argument block in use, at a ray count that fits the static quad
map and at one that needs the scheduler slot.  That build's outputs are tests/golden/g_render_launch_parent.npz
(tools/make_render_launch_golden.py, which also owns the cases and their inputs).

The render entries of the companion headers (the lean renders of the pair core, the coarse-weights renders, the lean fine launch) came later; the
entry layer of csrc/abi.hip above them decides nothing about what is computed either, and they are held the same way to
tests/golden/g_render_entries_parent.npz, recorded from the build before every render entry became one descriptor.

The large ray count is 4 * CUs + 6, so its hashes hold for the CU count they were recorded on: on another device those cases skip and say so.  The
small cases never skip."""
import importlib.util
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("make_render_launch_golden", os.path.join(ROOT, "tools", "make_render_launch_golden.py"))
G = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(G)


@pytest.fixture(scope="module")
def parent(golden):
    """(the recorded arrays, {case/output: SHA-256}, the CU count of the recording device)."""
    arrays = golden(os.path.splitext(os.path.basename(G.GOLDEN))[0])
    meta = json.loads(str(arrays["meta"]))
    return arrays, meta["sha256"], meta["cus"]


@pytest.fixture(scope="module")
def inputs():
    return G.Inputs(G.device_cus())


def _same(prefix, res, parent):
    arrays, shas, _ = parent
    assert sorted("%s/%s" % (prefix, k) for k in res) == sorted(k for k in shas if k.rsplit("/", 1)[0] == prefix), "%s: another set of outputs" % prefix
    for k, v in res.items():
        name, got = "%s/%s" % (prefix, k), G.words(v)
        if name in arrays:                       # an R = 6 case: the first word that differs (raw_*: the first sample point)
            want, have = arrays[name], G.stored(k, got)
            assert have.shape == want.shape and have.dtype == want.dtype, (name, have.shape, want.shape)
            diff = np.flatnonzero(have.ravel() != want.ravel())
            assert diff.size == 0, "%s differs from the recorded build in %d of %d %s, the first at %s: %#x, recorded %#x" % (
                name, diff.size, want.size, "rows" if k.startswith("raw_") else "words", np.unravel_index(diff[0], want.shape),
                int(have.ravel()[diff[0]]) & 0xffffffff, int(want.ravel()[diff[0]]) & 0xffffffff)
        assert G.sha(got) == shas[name], "%s differs from the recorded build (SHA-256 of its %d bytes)" % (name, got.nbytes)


@pytest.mark.parametrize("case", G.RENDER_CASES, ids=G.case_name)
def test_render_equals_the_recorded_build(case, inputs, parent):
    if case[2] == "large" and inputs.cus != parent[2]:
        pytest.skip("the fixture's large ray count is 4 * %d CUs + %d, this device has %d CUs" % (parent[2], G.SMALL_R, inputs.cus))
    res = G.run_render(inputs, case)
    assert res["feature_fine"].shape[0] == G.n_rays(case[2], inputs.cus)
    _same(G.case_name(case), res, parent)


@pytest.fixture(scope="module")
def parent_entries(golden):
    """The same of tests/golden/g_render_entries_parent.npz: the render entries of the companion headers, from the build before csrc/abi.hip described
    every render entry by one descriptor."""
    arrays = golden(os.path.splitext(os.path.basename(G.ENTRIES_GOLDEN))[0])
    meta = json.loads(str(arrays["meta"]))
    return arrays, meta["sha256"], meta["cus"]


@pytest.mark.parametrize("case", G.ENTRY_CASES, ids=G.case_name)
def test_companion_entry_equals_the_recorded_build(case, inputs, parent_entries):
    if case[2] == "large" and inputs.cus != parent_entries[2]:
        pytest.skip("the fixture's large ray count is 4 * %d CUs + %d, this device has %d CUs" % (parent_entries[2], G.SMALL_R, inputs.cus))
    res = G.run_entry(inputs, case)
    assert all(v.shape[0] == G.n_rays(case[2], inputs.cus) for v in res.values())
    _same(G.case_name(case), res, parent_entries)


@pytest.mark.parametrize("case", G.MLP_CASES, ids=G.case_name)
def test_mlp_forward_equals_the_recorded_build(case, inputs, parent):
    _same("mlp/" + G.case_name(case), G.run_mlp(inputs, case), parent)


def test_the_large_cases_need_the_scheduler_slot(inputs):
    """More ray quads than workgroups on this device, whatever its CU count: iters > 1 and the scheduler slot are in use."""
    assert (G.n_rays("large", inputs.cus) + 3) // 4 > inputs.cus
    assert (G.SMALL_R + 3) // 4 == 2 and G.SMALL_R % 4 != 0

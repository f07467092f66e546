"""The schedule of the fp32 core (csrc/mlp_core16.h: sub-stage stagger of the SIMD partners, LAG) changes WHEN a wave meets the weight ring's
barrier and issues its LDS-DMA pieces, never what it computes: every output of the inference kernels must equal, bit for bit, what the build
before the stagger returned.  That build's outputs are tests/golden/g_core16_parent.npz (tools/make_core16_golden.py, which also owns the cases
and their inputs).

A ring hazard shows as a wrong weight fragment, i.e. as wrong numbers, so the cases are the smallest shapes at which the stream can go wrong
(see RENDER_CASES there): a ragged quad, ragged last tiles, one-step passes where the stream turns from coarse to fine after a single walk, coarse
only, more quads than CUs (the dynamic quad counter, a second walk per workgroup) and the longest passes.  Each case runs with its weight stream
cold (a 256 MiB device copy right before the launch: the certification hazard is worst when the LDS-DMA is slow) and warm (back to back with the
previous launch: the refill hazard is worst when it is fast).  The training twins keep the unstaggered ring and are covered by their own tests."""
import importlib.util
import os

import numpy as np
import pytest
import torch

from crnerf_amd import ops

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("make_core16_golden", os.path.join(ROOT, "tools", "make_core16_golden.py"))
G = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(G)


@pytest.fixture(scope="module")
def parent(golden):
    """The recorded build's outputs (conftest's loader of tests/golden/)."""
    return golden(os.path.splitext(os.path.basename(G.GOLDEN))[0])


@pytest.fixture(scope="module")
def packs():
    return G.packs()


@pytest.fixture(scope="module")
def flusher():
    """Two 256 MiB device buffers; copying one to the other evicts the packed weights from every cache level in front of HBM."""
    a = torch.zeros(256 << 20, dtype=torch.uint8, device=G.DEV)
    b = torch.empty_like(a)
    return lambda: b.copy_(a)


def _same(name, key, got, parent):
    want = G.expand(name, key, parent["%s/%s" % (name, key)])
    got = got.cpu().numpy()
    assert got.shape == want.shape and got.dtype == want.dtype, (name, key, got.shape, want.shape)
    assert np.array_equal(got, want), "%s: %s differs from the recorded build in %d of %d places, max|d| %g" % (
        name, key, int((got != want).sum()), want.size, float(np.abs(got.astype(np.float64) - want).max()))


_RENDERED = {}


def _render(name, packs, flusher):
    """(cold, warm, (lean cold, lean warm) or None) of a case: rendered once, shared by the tests, never modified."""
    if name not in _RENDERED:
        R, nc, ni, _ = G.RENDER_CASES[name]
        rays, kw = G.render_inputs(name)
        with torch.no_grad():
            flusher()
            cold = ops.render_rays(packs[0], packs[1], rays, nc, ni, **kw)
            warm = ops.render_rays(packs[0], packs[1], rays, nc, ni, **kw)
            lean = None
            if ni > 0:                                 # the lean kernel runs the staggered ring too (124-stage coarse walks): cold, then warm
                flusher()
                lean = (ops.render_rays(packs[0], packs[1], rays, nc, ni, lean=True, **kw),
                        ops.render_rays(packs[0], packs[1], rays, nc, ni, lean=True, **kw))
        torch.cuda.synchronize()
        _RENDERED[name] = (cold, warm, lean)
    return _RENDERED[name]


@pytest.mark.parametrize("stream", ["cold", "warm"])
@pytest.mark.parametrize("name", list(G.RENDER_CASES))
def test_render_equals_the_recorded_build(name, stream, packs, flusher, parent):
    res = _render(name, packs, flusher)[0 if stream == "cold" else 1]
    ni = G.RENDER_CASES[name][2]
    assert sorted(res) == sorted(G.RENDER_KEYS if ni > 0 else G.RENDER_KEYS[:3])
    for k in res:
        _same(name, k, res[k], parent)


def test_more_quads_than_cus(packs):
    """The many-quads case is what its name says on this device: every workgroup pulls from the quad counter, some walk twice."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert (G.RENDER_CASES["more_quads_than_cus_1032x8+8"][0] + 3) // 4 > cus


@pytest.mark.parametrize("name", [n for n, c in G.RENDER_CASES.items() if c[2] > 0])
def test_lean_equals_full_and_the_recorded_build(name, packs, flusher, parent):
    cold, _, leans = _render(name, packs, flusher)
    for lean in leans:                                 # cold weight stream, then back to back
        assert sorted(lean) == ["depth_fine", "feature_fine", "z_fine"]
        for k in lean:
            assert torch.equal(lean[k], cold[k]), (name, k)
            _same(name, k, lean[k], parent)


@pytest.mark.parametrize("name", list(G.MLP_CASES))
def test_mlp_forward_equals_the_recorded_build(name, packs, flusher, parent):
    x = G.mlp_inputs(name)
    with torch.no_grad():
        flusher()
        cold = ops.mlp_forward(packs[0], x)
        warm = ops.mlp_forward(packs[0], x)
    torch.cuda.synchronize()
    _same(name, "out", cold, parent)
    _same(name, "out", warm, parent)


def test_rng_kernel_equals_the_recorded_build(packs, flusher, parent):
    name, R, nc, ni, rng = G.RNG_CASE
    rays, kw = G.render_inputs(name)
    with torch.no_grad():
        flusher()
        cold = ops.render_rays(packs[0], packs[1], rays, nc, ni, noise_std=1.0, rng=rng, **kw)
        warm = ops.render_rays(packs[0], packs[1], rays, nc, ni, noise_std=1.0, rng=rng, **kw)
    torch.cuda.synchronize()
    assert "z_coarse_used" in cold and "noise_fine_used" in cold
    for res in (cold, warm):
        for k in res:
            _same(name, k, res[k], parent)

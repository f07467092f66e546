"""models/rendering.py::render_rays_cross_ray against tests/golden/render_routes.json (tools/make_render_route_golden.py: recorded from the function
while it chose its launch in one if / elif chain): every row reaches the recorded launch seams with the recorded arguments, draws included, and names
its result as recorded; and render_route(), asked directly with a row's plain values, names the path whose seam the row then hits.  No GPU and no
libcrnerf_hip.so needed."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_render_route_golden as G  # noqa: E402

from crnerf_amd import _lib, autograd  # noqa: E402
from crnerf_amd.models import rendering  # noqa: E402
from crnerf_amd.precision import resolve  # noqa: E402

# the seams a path ends in (NeRF_sigma.packed_weights aside)
SEAMS_OF = {"train_fused": [["fused_render_with_grad"]], "unfused": [["_render_unfused"]], "lean_x": [["render_rays_lean_x"]], "fused": [["render_rays"]],
            "composite": [["render_rays", "render_rays_bf16_fine"], ["render_coarse_weights", "render_rays_bf16_fine"]]}


@pytest.fixture(scope="module")
def table():
    with open(G.GOLDEN) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def replayed():
    """[(row, its outcome now, the RenderRoute render_route gives its plain values -- None for a grad-mode lean row, which is refused before)],
    made with _lib.load() refusing to work: neither the replay nor render_route may ask for libcrnerf_hip.so (another module of the same process may
    have loaded it before; _lib._lib is then what it was)."""
    def refuse():
        raise AssertionError("the front door asked for libcrnerf_hip.so")
    out, before, load = [], _lib._lib, _lib.load
    _lib.load = refuse
    try:
        _replay_all(out)
    finally:
        _lib.load = load
    assert _lib._lib is before
    return out


def _replay_all(out):
    with G.seams() as s:
        for row in G.rows():
            train = row["grad"] and not row["frozen"]
            route = None
            if not (train and row["lean"]):
                with G.settings(row):
                    route = rendering.render_route(resolve(row["precision"], composite=True), train, autograd.training_plan() if train else None,
                                                   row["jitter"], row["perturb"], row["noise_std"], row["Nc"], row["Ni"], row["lean"], row["rng"])
            out.append((row, G.replay(s, row), route))


def test_the_rows_are_the_recorded_rows(table):
    n = len(G.N_SAMPLES) * len(G.N_IMPORTANCE) * len(G.PRECISIONS) * 2 ** 6     # the full product; the factored rows follow it
    assert len(G.rows()) == len(table["rows"]) > n == 8192 and os.path.getsize(G.GOLDEN) < 200_000
    assert len({json.dumps(r, sort_keys=True) for r in G.rows()}) == len(G.rows())


def test_every_row_replays_to_the_recorded_outcome(table, replayed):
    for i, (row, got, _) in enumerate(replayed):
        assert G.canonical(got) == G.canonical(G.expand(table, i)), (i, row)


def test_feature_fine_random_is_feature_fine(replayed):
    seen = 0
    for row, got, _ in replayed:
        names = dict(got.get("returns", []))
        if "feature_fine_random" in names:
            seen += 1
            assert names["feature_fine_random"] == names["feature_fine"], row
            assert row["output_random"] and row["encode_random"] and row["Ni"] > 0
    assert seen > 1000


def test_render_route_names_the_path_the_row_takes(replayed):
    paths = set()
    for row, got, route in replayed:
        if route is None:
            assert got["raises"][0] == "ValueError" and not got["calls"], row
            continue
        assert "raises" not in got, (row, got)
        launches = [seam for seam, _ in got["calls"] if seam != "packed_weights"]
        assert launches in SEAMS_OF[route.path], (row, route, launches)
        last = got["calls"][-1][1]
        # the route's other fields are what the launch was handed
        if route.path in ("fused", "composite"):
            assert last["lean"] is route.lean_launch, (row, route)
        if route.path == "composite":
            assert (launches[0] == "render_coarse_weights") is route.lean_launch and (got["calls"][0][1]["precision"] == "f16") is route.f16_coarse
        else:
            assert route.path == "train_fused" or last["precision"] == route.precision, (row, route)
        assert (last.get("rng") is not None) is route.kernel_draws, (row, route)
        assert route.lean is ("weights_%s" % ("fine" if row["Ni"] else "coarse") not in dict(got["returns"])), (row, route)
        paths.add((route.path, route.lean, route.lean_launch, route.f16_coarse, route.kernel_draws))
    assert {p[0] for p in paths} == set(SEAMS_OF) and len(paths) >= 12


def test_a_route_is_immutable_and_pure():
    a = rendering.render_route("bf16_hc", False, None, False, 0, 1, 64, 128, True, True)
    assert a == ("composite", "bf16", True, True, False, False) and a == rendering.render_route("bf16_hc", False, None, False, 0, 1, 64, 128, True, False)
    with pytest.raises(AttributeError):
        a.path = "fused"
    # the row ADVICE.md names, unchanged: "bf16_hc" keeps its two-launch path beyond N_importance = 256, "bf16_fc" renders un-fused there
    assert rendering.render_route("bf16_hc", False, None, False, 0, 0, 64, 257, False, True).path == "composite"
    assert rendering.render_route("bf16_fc", False, None, False, 0, 0, 64, 257, False, True)[:2] == ("unfused", "bf16")

"""lean=True on the fp32-accurate split cores: crnerf_render_rays_lean_f32x3 / _f32h2 / _f32x3_repair (include/crnerf_lean_x.h;
ops.render_rays_lean_x) and the route to them from render_rays_cross_ray under precision "f32x3", "f32h2" and "auto".

The lean kernel is the full kernel minus work nobody reads: its coarse tiles walk layers 1..8 and static_sigma (the weight ring fetches the shorter
walk for them and the whole stream for the fine tiles), alpha, the scan and the weights execute the full kernel's arithmetic in its order, the fine
pass is the full kernel's, and only feature_fine, depth_fine and z_fine are stored.  So every comparison against the full call is torch.equal -- a
property by construction, not a tolerance.  Each shape is one way the alternating walk, the ring phase or the quad logic could go wrong."""
import pytest
import torch

import _lean_x_cases as K
from crnerf_amd import _lib, ops

pytestmark = pytest.mark.gpu
DEV = K.DEV
KEYS = ["feature_fine", "depth_fine", "z_fine"]
MARK = 0x7fc00000


def _many():
    """4 * CUs + 5 rays: every workgroup renders at least two quads -- fine tile -> the next ray's trunk tile -- and the last quad is ragged."""
    return 4 * torch.cuda.get_device_properties(0).multi_processor_count + 5


# (R or a function of the device, Nc, Ni, use_disp)
CASES = {
    "minimum_8x3+1": (8, 3, 1, False),
    "partial_coarse_tile_8x33+31_disp": (8, 33, 31, True),            # a partly filled coarse tile, Nf = 64
    "8x64+128": (8, 64, 128, False),
    "maximum_8x256+256_disp": (8, 256, 256, True),
    "ragged_quad_5x33+31": (5, 33, 31, False),
    "two_quads_per_workgroup_x33+31": (_many, 33, 31, False),
}
_RUNS = {}


def both(precision, name):
    """(rays, keywords, full render, lean render) of a case; rendered once and shared, never modified."""
    if (precision, name) not in _RUNS:
        R, nc, ni, disp = CASES[name]
        rays, kw = K.inputs(R() if callable(R) else R, nc, ni, disp)
        pc, pf = K.packs(precision)
        with torch.no_grad():
            full = ops.render_rays(pc, pf, rays, nc, ni, precision=precision, **kw)
            lean = ops.render_rays_lean_x(pc, pf, rays, nc, ni, precision=precision, **kw)
        torch.cuda.synchronize()
        _RUNS[(precision, name)] = (rays, kw, full, lean)
    return _RUNS[(precision, name)]


@pytest.mark.parametrize("name", list(CASES))
@pytest.mark.parametrize("precision", ["f32x3", "f32h2"])
def test_lean_equals_the_full_render_bit_for_bit(precision, name):
    rays, _, full, lean = both(precision, name)
    _, nc, ni, _ = CASES[name]
    assert list(lean) == KEYS                                            # nothing else is allocated
    assert lean["feature_fine"].shape == (rays.shape[0], 64) and lean["depth_fine"].shape == (rays.shape[0],) and lean["z_fine"].shape == (rays.shape[0], nc + ni)
    assert bool(torch.isfinite(full["feature_fine"]).all()) and float(full["feature_fine"].abs().sum()) > 0
    for k in KEYS:
        assert torch.equal(lean[k], full[k]), "%s %s: %s differs in %d of %d places, max|d| %g" % (
            precision, name, k, int((lean[k] != full[k]).sum()), full[k].numel(), float((lean[k] - full[k]).abs().max()))


@torch.no_grad()
@pytest.mark.parametrize("name", ["8x64+128", "two_quads_per_workgroup_x33+31"])
def test_auto_without_trouble_is_the_h2_render_and_the_repair_changes_nothing(name):
    rays, kw, _, lean_h2 = both("f32h2", name)
    _, nc, ni, _ = CASES[name]
    pc, pf = K.packs("auto")
    auto = ops.render_rays_lean_x(pc, pf, rays, nc, ni, precision="auto", **kw)
    torch.cuda.synchronize()
    assert list(auto) == KEYS
    for k in KEYS:
        assert torch.equal(auto[k], lean_h2[k]), k


# ---------------------------------------------------------------- the mark and its repair
def _bits_equal(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)) if a.numel() else True


def _quads(marked):
    return marked.view(-1, 4).any(1)[:, None].expand(-1, 4).reshape(-1)


def _check_marked_rows_and_repair(lean_h2, lean_x3, auto, full_h2, marked):
    """What the marked-ray cases share: a marked feature row is NaN throughout, every other row is the full call's, and "auto" returns the x3 core's
    rows for the quads with a marked ray and the h2 core's for the others."""
    assert 0 < int(marked.sum()) and not bool(_quads(marked).all())                  # the case cannot pass empty
    assert bool(torch.isnan(lean_h2["feature_fine"][marked]).all())
    for k in ("feature_fine", "depth_fine"):
        assert bool(torch.isfinite(lean_h2[k][~marked]).all()), k
        assert torch.equal(lean_h2[k][~marked], full_h2[k][~marked]), k
    quad = _quads(marked)
    assert bool(torch.isfinite(lean_x3["feature_fine"]).all())
    for k in ("feature_fine", "depth_fine"):
        assert torch.equal(auto[k][quad], lean_x3[k][quad]), k
        assert torch.equal(auto[k][~quad], lean_h2[k][~quad]), k


def _overflow_runs(coarse, fine):
    R, nc, ni = 256, 64, 64
    rays = K.overflow_rays()
    kw = dict(z_steps=torch.linspace(0, 1, nc, device=DEV), u=torch.linspace(0, 1, ni, device=DEV))
    out = {p: ops.render_rays_lean_x(*K.packs(p, coarse, fine), rays, nc, ni, precision=p, **kw) for p in ("f32h2", "f32x3", "auto")}
    out["full"] = ops.render_rays(*K.packs("f32h2", coarse, fine), rays, nc, ni, precision="f32h2", **kw)
    out["cw"] = ops.render_coarse_weights(K.packs("f32h2", coarse, fine)[0], rays, nc, precision="f32h2", z_steps=kw["z_steps"])["weights_coarse"]
    torch.cuda.synchronize()
    assert R == rays.shape[0]
    return out


@torch.no_grad()
def test_coarse_side_marks_and_their_repair():
    K.auto_pack("over", K.overflow_state())
    o = _overflow_runs("over", "f")
    marked = torch.isnan(o["f32h2"]["feature_fine"]).any(1)
    expected = (o["cw"][:, 0].view(torch.int32) == MARK) | torch.isnan(o["full"]["feature_fine"][:, 0])
    print("coarse side: %d rays marked, %d by the coarse-weights render, %d NaN in the full render" % (
        int(marked.sum()), int((o["cw"][:, 0].view(torch.int32) == MARK).sum()), int(torch.isnan(o["full"]["feature_fine"][:, 0]).sum())))
    assert torch.equal(marked, expected)
    assert bool(torch.isnan(o["f32h2"]["depth_fine"][marked]).all())                   # the coarse-side mark: the whole row and the depth
    _check_marked_rows_and_repair(o["f32h2"], o["f32x3"], o["auto"], o["full"], marked)


@torch.no_grad()
def test_fine_side_marks_and_their_repair():
    K.auto_pack("over", K.overflow_state())
    o = _overflow_runs("c", "over")
    marked = torch.isnan(o["f32h2"]["feature_fine"]).any(1)
    assert not bool((o["cw"][:, 0].view(torch.int32) == MARK).any())                   # nothing trips on the coarse side here
    assert torch.equal(marked, torch.isnan(o["full"]["feature_fine"]).any(1))
    # a fine-side trip is the full kernel's own: the poisoned point's features reach the row, its weight is 0 (the unit is built with -fno-honor-nans:
    # max(NaN, 0) = 0), so the depth stays finite -- the lean kernel returns the full kernel's bits, marked rows included
    for k in ("feature_fine", "depth_fine"):
        assert _bits_equal(o["f32h2"][k], o["full"][k]), k
    _check_marked_rows_and_repair(o["f32h2"], o["f32x3"], o["auto"], o["full"], marked)


@torch.no_grad()
def test_a_pack_with_the_range_flag_marks_every_ray_and_auto_renders_on_x3():
    flagged, fine = K.flagged_pack(), K.auto_pack("f")
    R, nc, ni = 8, 33, 31
    rays, kw = K.inputs(R, nc, ni, False)
    h2 = ops.render_rays_lean_x(flagged.h2, fine.h2, rays, nc, ni, precision="f32h2", **kw)
    assert bool(torch.isnan(h2["feature_fine"][:, 0]).all())
    auto = ops.render_rays_lean_x(flagged, fine, rays, nc, ni, precision="auto", **kw)
    x3 = ops.render_rays_lean_x(flagged.x3, fine.x3, rays, nc, ni, precision="f32x3", **kw)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(x3["feature_fine"]).all())
    for k in ("feature_fine", "depth_fine"):
        assert torch.equal(auto[k], x3[k]), k


# ---------------------------------------------------------------- nothing else allocated
@torch.no_grad()
@pytest.mark.parametrize("precision", ["f32h2", "auto"])
def test_lean_call_allocates_its_three_outputs_and_nothing_else(precision):
    """A condition, not a measurement.  Every tensor of the case is a multiple of 4,096 bytes below 1 MiB, so the caching allocator hands out exactly
    what is asked for: the lean call's peak above its inputs is 4 R (64 + 1) bytes plus z_fine, the full call's larger by
    4 R (64 + 1 + Nc + Nc + Ni) -- feature_coarse, depth_coarse, weights_coarse, weights_fine."""
    R, nc, ni = 1024, 33, 31
    rays, kw = K.inputs(R, nc, ni, False)
    pc, pf = K.packs(precision)
    peaks = {}
    for lean in (False, True):
        call = (lambda: ops.render_rays_lean_x(pc, pf, rays, nc, ni, precision=precision, **kw)) if lean else \
               (lambda: ops.render_rays(pc, pf, rays, nc, ni, precision=precision, **kw))
        call()
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        out = call()
        torch.cuda.synchronize()
        peaks[lean] = torch.cuda.max_memory_allocated() - base
        del out
    print("%s: peak of the full call %d bytes, of the lean call %d bytes" % (precision, peaks[False], peaks[True]))
    assert peaks[True] == 4 * R * (64 + 1) + 4 * R * (nc + ni)
    assert peaks[False] - peaks[True] == 4 * R * (64 + 1 + nc + nc + ni)


# ---------------------------------------------------------------- through the mirror
class _Args:
    nerf_out_dim, img_wh, pertubeCord = 64, [24, 20], False
    N_samples, N_importance, use_disp = 64, 128, False


@pytest.fixture(scope="module")
def scene():
    from crnerf_amd.models.nerf import NeRF_sigma, PosEmbedding
    args = _Args()
    models = {"coarse": NeRF_sigma("coarse", args, in_channels_xyz=93, in_channels_dir=27).to(DEV),
              "fine": NeRF_sigma("fine", args, in_channels_xyz=93, in_channels_dir=27, encode_random=True).to(DEV)}
    models["coarse"].load_state_dict({k: torch.from_numpy(v) for k, v in K.ST_C.items()})
    models["fine"].load_state_dict({k: torch.from_numpy(v) for k, v in K.ST_F.items()})
    emb = {"xyz": PosEmbedding(14, 15), "dir": PosEmbedding(3, 4)}
    return args, models, emb


LEAN_KEYS = ["feature_fine", "feature_fine_random", "depth_fine"]
FULL_KEYS = ["weights_coarse", "feature_coarse", "depth_coarse", "weights_fine", "feature_fine", "feature_fine_random", "depth_fine"]
ROUTES = {"f32x3": (["crnerf_render_rays_f32x3"], ["crnerf_render_rays_lean_f32x3"]),
          "f32h2": (["crnerf_render_rays_f32h2"], ["crnerf_render_rays_lean_f32h2"]),
          "auto": (["crnerf_render_rays_f32h2", "crnerf_render_rays_f32x3_repair"], ["crnerf_render_rays_lean_f32h2", "crnerf_render_rays_lean_f32x3_repair"])}


@torch.no_grad()
@pytest.mark.parametrize("perturb", [0, 1])
@pytest.mark.parametrize("precision", list(ROUTES))
def test_mirror_takes_the_lean_entries_and_returns_the_full_values(scene, precision, perturb, monkeypatch):
    """The test that fails without the feature: on the parent the mirror switches the flag off for these precisions, calls the full entry and drops keys."""
    from crnerf_amd.models.rendering import render_rays_cross_ray
    args, models, emb = scene
    lib, calls = _lib.load(), []
    for name in set(sum((a + b for a, b in ROUTES.values()), [])):
        def spy(*a, _real=getattr(lib, name), _name=name):
            calls.append(_name)
            return _real(*a)
        monkeypatch.setattr(lib, name, spy)
    rays = K.C(K.synth.rays(40, seed=5, H=5, W=8))

    def call(**kw):
        torch.manual_seed(11)          # perturb = 1: the jitter, the uniforms and the density noise arrive as tensors, the same ones in both calls
        del calls[:]
        out = render_rays_cross_ray(models, emb, rays, None, 64, False, perturb, float(perturb), 128, 4096, False, test_time=True, args=args,
                                    precision=precision, **kw)
        return out, list(calls)
    full, full_calls = call()
    lean, lean_calls = call(lean=True)
    torch.cuda.synchronize()
    assert full_calls == ROUTES[precision][0] and lean_calls == ROUTES[precision][1]
    assert list(full) == FULL_KEYS and list(lean) == LEAN_KEYS and lean["feature_fine_random"] is lean["feature_fine"]
    assert bool(torch.isfinite(full["feature_fine"]).all())
    for k in LEAN_KEYS:
        assert torch.equal(lean[k], full[k]), k


@torch.no_grad()
@pytest.mark.parametrize("lean", [False, True])
@pytest.mark.parametrize("precision", ["f32", "auto"])
def test_mirror_hands_on_the_draws_it_makes(scene, precision, lean):
    """The draws the mirror makes on the device -- _coarse_depths, u, noise_c, noise_f, in that order -- are the tensors its launch gets: drawn again
    from the same seed and handed to the entry the route names, they give the same bits.  Six rays: two ray quads, the second partial."""
    from crnerf_amd.models import rendering
    args, models, emb = scene
    R, nc, ni = 6, 5, 4
    rays = K.C(K.synth.rays(R, seed=5, H=2, W=3))
    torch.manual_seed(0)
    got = rendering.render_rays_cross_ray(models, emb, rays, None, nc, False, 1, 1, ni, 4096, False, test_time=True, args=args, precision=precision, lean=lean)
    torch.manual_seed(0)
    z = rendering._coarse_depths(rays, nc, False, 1)
    u = torch.rand(R, ni, device=rays.device)
    noise_c = torch.randn(R, nc, device=rays.device)
    noise_f = torch.randn(R, nc + ni, device=rays.device)
    launch = dict(precision=precision, z_coarse=z, z_steps=torch.linspace(0, 1, nc, device=rays.device), u=u, noise_coarse=noise_c, noise_fine=noise_f,
                  noise_std=1.0)
    packs = [models[k].packed_weights(precision) for k in ("coarse", "fine")]
    if lean and precision == "auto":
        want = ops.render_rays_lean_x(*packs, rays, nc, ni, **launch)
    else:
        want = ops.render_rays(*packs, rays, nc, ni, lean=lean, **launch)
    torch.cuda.synchronize()
    assert list(got) == (LEAN_KEYS if lean else FULL_KEYS) and bool(torch.isfinite(got["feature_fine"]).all())
    for k in got:
        assert torch.equal(got[k], want["feature_fine" if k == "feature_fine_random" else k]), k

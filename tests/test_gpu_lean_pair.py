"""The lean inference render on the pair core (crnerf_render_rays_lean_bf16 / _f16; ops.render_rays(..., lean=True, precision="bf16" | "f16");
render_rays_cross_ray(..., lean=True)).

The lean kernel is the full pair-core kernel minus work nobody reads: its coarse tiles walk the trunk (992 of the 1,208 fragments of the weight
stream, 62 ring stages = half a ring turn more than a whole number), no coarse feature is composited, nothing of the coarse pass and no
weights_fine reach HBM.  The trunk, the sigma head, the compositing scan, sample_pdf, the merge and the fine pass execute the full kernel's
instructions in the full kernel's order, so feature_fine, depth_fine and z_fine are compared with torch.equal -- a property by construction, not
a tolerance.  Every shape is one way the ring phase or the quad logic could go wrong (see CASES).  The ring's protocol itself is proved by the
static_asserts of csrc/mlp_core_bf16p.h, not here."""
import ctypes

import numpy as np
import pytest
import torch

import crnerf_amd.synth as synth
from crnerf_amd import _lib, ops, pipeline
from oracle import cpu_ref as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PRECISIONS = ["bf16", "f16"]
ST_C, ST_F = synth.mlp_state(5, 3.0, 1.0), synth.mlp_state(6, 3.0, 1.0)      # tests/test_gpu_lean.py's states; largest |weight| 1.2: they pack for fp16
KEYS = ("z_fine", "depth_fine", "feature_fine")


def C(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


_PACKS = {}


def packs(precision):
    if precision not in _PACKS:
        pk = lambda st: ops.pack_mlp_weights({k: C(v) for k, v in st.items()}, precision=precision)  # noqa: E731
        _PACKS[precision] = (pk(ST_C), pk(ST_F))
    return _PACKS[precision]


def _inputs(R, nc, ni, disp, rich):
    rays = synth.rays(R, seed=3)
    kw = dict(use_disp=disp, z_steps=torch.linspace(0, 1, nc).to(DEV), u=torch.linspace(0, 1, ni).to(DEV), want_z_fine=True)
    if rich:       # everything the training-time path hands over as tensors: view_dir, density noise, caller's coarse depths, per-ray u
        rng = np.random.default_rng(4)
        vd = rng.normal(size=(R, 3)).astype(np.float32)
        vd /= np.linalg.norm(vd, axis=-1, keepdims=True)
        kw.update(view_dir=C(vd), z_coarse=C(np.sort(rng.uniform(rays[:, 6:7], rays[:, 7:8], (R, nc)).astype(np.float32), -1)),
                  u=C(rng.uniform(0, 1, (R, ni)).astype(np.float32)), noise_coarse=C(rng.normal(size=(R, nc)).astype(np.float32)),
                  noise_fine=C(rng.normal(size=(R, nc + ni)).astype(np.float32)), noise_std=1.0)
        del kw["z_steps"]
    return C(rays), kw


CASES = {
    "ragged_quad_5x64+128": (5, 64, 128, False, False),           # a ragged last ray quad
    "dynamic_sched_1030x64+128": (1030, 64, 128, False, False),   # 258 quads on 256 CUs: the device-side quad counter; trunk / full walks alternate across quads
    "one_step_8x3+5_disp": (8, 3, 5, True, False),                # one coarse step: wave B of each pair holds no valid sample; the ring phase flips per ray
    "one_step_8x33+31_disp": (8, 33, 31, True, False),            # one coarse step, one fine step
    "two_steps_8x96+40": (8, 96, 40, False, False),               # two coarse steps, the second half-empty; three fine steps
    "odd_steps_8x160+96": (8, 160, 96, False, False),             # THREE coarse steps: the fine pass and the next ray start half a ring turn on
    "maximum_8x256+256": (8, 256, 256, False, False),             # 4 trunk walks then 8 full ones
    "tensors_64x48+40": (64, 48, 40, False, True),                # view_dir, noise tensors, noise_std = 1, caller's z_coarse, per-ray u
}
_REF = {}


def _both(precision, name):
    """(inputs, full render, lean render) of a case; rendered once and shared, never modified."""
    if (precision, name) not in _REF:
        R, nc, ni, disp, rich = CASES[name]
        rays, kw = _inputs(R, nc, ni, disp, rich)
        pc, pf = packs(precision)
        with torch.no_grad():
            full = ops.render_rays(pc, pf, rays, nc, ni, precision=precision, **kw)
            lean = ops.render_rays(pc, pf, rays, nc, ni, precision=precision, lean=True, **kw)
        torch.cuda.synchronize()
        _REF[(precision, name)] = (rays, kw, full, lean)
    return _REF[(precision, name)]


def _assert_equal(got, want, what):
    for k in KEYS:
        assert torch.equal(got[k], want[k]), "%s: %s differs in %d places, max|d| %g" % (
            what, k, int((got[k] != want[k]).sum()), float((got[k] - want[k]).abs().max()))


@pytest.mark.parametrize("name", list(CASES))
@pytest.mark.parametrize("precision", PRECISIONS)
def test_lean_equals_full_bit_for_bit(precision, name):
    _, _, full, lean = _both(precision, name)
    assert sorted(lean) == ["depth_fine", "feature_fine", "z_fine"]
    assert bool(torch.isfinite(full["feature_fine"]).all())
    _assert_equal(lean, full, "%s %s" % (precision, name))


@pytest.mark.parametrize("precision", PRECISIONS)
def test_back_to_back_lean_launches_leave_the_scheduler_words_zeroed(precision):
    """Two lean launches and a full one on the same stream, nothing in between: every one of them takes the dynamic quad counter from zero."""
    name = "dynamic_sched_1030x64+128"
    rays, kw, full, _ = _both(precision, name)
    R, nc, ni = CASES[name][:3]
    pc, pf = packs(precision)
    with torch.no_grad():
        a = ops.render_rays(pc, pf, rays, nc, ni, precision=precision, lean=True, **kw)
        b = ops.render_rays(pc, pf, rays, nc, ni, precision=precision, lean=True, **kw)
        c = ops.render_rays(pc, pf, rays, nc, ni, precision=precision, **kw)
    torch.cuda.synchronize()
    _assert_equal(a, full, "first lean launch")
    _assert_equal(b, full, "second lean launch")
    for k in full:
        assert torch.equal(c[k], full[k]), k


@pytest.mark.parametrize("precision", PRECISIONS)
def test_cold_weights_once(precision):
    """32,768 rays with the weight streams evicted from L2 (a 1 GiB copy, as tests/test_gpu_bf16.py::test_render_cold_l2_is_deterministic does it)
    in front of the lean call: one cold and one warm lean render, both bit-equal to the full render.  One shot, not a hunt: the ring's protocol
    is proved at compile time."""
    R, nc, ni = 32768, 64, 128
    pc, pf = packs(precision)
    rays = C(synth.rays(R, seed=0, H=128, W=256))
    kw = dict(z_steps=torch.linspace(0, 1, nc, device=DEV), u=torch.linspace(0, 1, ni, device=DEV), want_z_fine=True, precision=precision)
    with torch.no_grad():
        full = ops.render_rays(pc, pf, rays, nc, ni, **kw)
        junk_a, junk_b = torch.empty(1 << 28, device=DEV), torch.zeros(1 << 28, device=DEV)   # 1 GiB each: far beyond L2 + MALL
        junk_a.copy_(junk_b)
        cold = ops.render_rays(pc, pf, rays, nc, ni, lean=True, **kw)
        warm = ops.render_rays(pc, pf, rays, nc, ni, lean=True, **kw)
    torch.cuda.synchronize()
    _assert_equal(cold, full, "cold lean render")
    _assert_equal(warm, full, "warm lean render")


def _err(got, want):
    d = (got.detach().double().cpu() - torch.as_tensor(want).double()).abs()
    return float(d.max()), float(d.mean())


@pytest.mark.parametrize("precision", PRECISIONS)
def test_lean_against_the_oracle(precision):
    """The R = 64 case (view_dir, noise, caller's depths, per-ray u): the fine pass against the oracle's emulation of the precision at the kernel's
    own fine depths, with the bars tests/test_gpu_bf16.py / tests/test_gpu_f16.py hold the fused render to (max 2e-2, mean 2e-4)."""
    import contextlib
    from test_gpu_f16 import f16_emulation
    rays, kw, _, lean = _both(precision, "tensors_64x48+40")
    r, zf = rays.cpu(), lean["z_fine"].cpu()
    assert bool((zf[:, 1:] >= zf[:, :-1]).all())
    with (f16_emulation() if precision == "f16" else contextlib.nullcontext()):
        raw = O._run_model(O.to_torch(ST_F), r, zf, O.posenc(kw["view_dir"].cpu(), 4), 32768, mlp=O.mlp_forward_bf16)
    _, f2, d2 = O.composite(raw, zf, kw["noise_fine"].cpu(), 1.0)
    for k, want in (("feature_fine", f2), ("depth_fine", d2)):
        mx, mean = _err(lean[k], want)
        print("lean %s vs emulation, %s: max %.3e mean %.3e" % (precision, k, mx, mean))
        assert mx < 2e-2 and mean < 2e-4, (k, mx, mean)


@torch.no_grad()
def test_f16_range_guard_marks_the_fine_row():
    """tests/test_gpu_f16.py's guard case (a coarse model whose xyz_encoding_8 output leaves fp16's range on some rays) with a fine model behind it.
    The full kernel marks such a ray by a NaN feature_coarse row and returns finite fine numbers sampled from a wrong pdf; the lean kernel has no
    feature_coarse, so the mark is the fine row itself: all 64 features and the depth NaN.  Every other ray: bit-identical."""
    from test_gpu_f16 import _guard_case
    st, rays, over, zt = _guard_case()
    Nc, Ni = 64, 128
    pk = lambda s: ops.pack_mlp_weights({k: C(v) for k, v in s.items()}, precision="f16")  # noqa: E731
    pc, pf = pk(st), pk(synth.mlp_state(22, 2.0))
    kw = dict(z_steps=zt.to(DEV), u=torch.linspace(0, 1, Ni, device=DEV), want_z_fine=True, precision="f16")
    full = ops.render_rays(pc, pf, rays.to(DEV), Nc, Ni, **kw)
    lean = ops.render_rays(pc, pf, rays.to(DEV), Nc, Ni, lean=True, **kw)
    tripped = torch.isnan(full["feature_coarse"]).any(1)
    print("lean range guard: %d rays, %d overflow in the emulation, %d marked by the full kernel" % (len(over), int(over.sum()), int(tripped.sum())))
    assert torch.equal(tripped.cpu(), over)
    assert int(tripped.sum()) >= 8 and int((~tripped).sum()) >= 8
    assert bool(torch.isnan(lean["feature_fine"][tripped]).all()) and bool(torch.isnan(lean["depth_fine"][tripped]).all())
    ok = ~tripped
    assert bool(torch.isfinite(full["feature_fine"][ok]).all())
    for k in KEYS:
        assert torch.equal(lean[k][ok], full[k][ok]), k


def _args(pk, rays, nc, ni, out):
    a = _lib.RenderArgs()
    a.packed_coarse, a.packed_fine, a.rays = pk[0].data_ptr(), pk[1].data_ptr(), rays.data_ptr()
    a.n_rays, a.n_samples, a.n_importance = rays.shape[0], nc, ni
    a.feature_fine, a.depth_fine = out["feature_fine"].data_ptr(), out["depth_fine"].data_ptr()
    return a


@pytest.mark.parametrize("precision", PRECISIONS)
def test_entry_points_directly(precision):
    lib = _lib.load()
    pk = packs(precision)
    rays = _both(precision, "ragged_quad_5x64+128")[0]
    out = {"feature_fine": torch.zeros(5, 64, device=DEV), "depth_fine": torch.zeros(5, device=DEV), "z_coarse_used": torch.zeros(5, 64, device=DEV)}
    fn = getattr(lib, "crnerf_render_rays_lean_" + precision)
    call = lambda a: fn(ctypes.byref(a), _lib.stream_ptr())  # noqa: E731
    assert call(_args(pk, rays, 64, 0, out)) == -2                # CRNERF_ERR_SHAPE
    assert call(_args(pk, rays, 2, 128, out)) == -2
    assert call(_args(pk, rays, 257, 128, out)) == -2
    a = _args(pk, rays, 64, 128, out)
    a.rng_flags = 1
    assert call(a) == -3                                          # CRNERF_ERR_CONFIG
    a = _args(pk, rays, 64, 128, out)
    a.z_coarse_out = out["z_coarse_used"].data_ptr()
    assert call(a) == -3
    a = _args(pk, rays, 64, 128, out)
    a.packed_fine = None
    assert call(a) == -1
    torch.cuda.synchronize()
    assert float(out["feature_fine"].abs().max()) == 0.0 and float(out["depth_fine"].abs().max()) == 0.0     # a refused call launched nothing
    # NULL weights_* / feature_coarse / depth_coarse / z_fine / z_steps / u are accepted; in-kernel linspace tables in both kernels
    assert call(_args(pk, rays, 64, 128, out)) == 0
    ref = ops.render_rays(pk[0], pk[1], rays, 64, 128, precision=precision)
    torch.cuda.synchronize()
    assert torch.equal(out["feature_fine"], ref["feature_fine"]) and torch.equal(out["depth_fine"], ref["depth_fine"])
    with pytest.raises(ValueError):
        ops.render_rays(pk[0], pk[1], rays, 64, 128, lean=True, train=True, precision=precision)


# ---------------------------------------------------------------- through the mirror
class _Args:
    nerf_out_dim, img_wh, pertubeCord = 64, [16, 12], False


@pytest.fixture(scope="module")
def scene():
    from crnerf_amd.models.linearStyleTransfer import style_net
    from crnerf_amd.models.nerf import NeRF_sigma, PosEmbedding
    args = _Args()
    models = {"coarse": NeRF_sigma("coarse", args, in_channels_xyz=93, in_channels_dir=27).to(DEV),
              "fine": NeRF_sigma("fine", args, in_channels_xyz=93, in_channels_dir=27, encode_random=True).to(DEV),
              "decoder": style_net(args).to(DEV)}
    models["coarse"].load_state_dict({k: torch.from_numpy(v) for k, v in ST_C.items()})
    models["fine"].load_state_dict({k: torch.from_numpy(v) for k, v in ST_F.items()})
    models["decoder"].load_state_dict({k: torch.from_numpy(v) for k, v in synth.decoder_state(31).items()})
    emb = {"xyz": PosEmbedding(14, 15), "dir": PosEmbedding(3, 4)}
    rays = C(synth.rays(16 * 12, seed=5, H=12, W=16))
    style = C(np.random.default_rng(1).uniform(0, 1, (1, 64, 32, 32)).astype(np.float32))
    return args, models, emb, rays, style


LEAN_KEYS = ["feature_fine", "feature_fine_random", "depth_fine"]
FULL_KEYS = ["weights_coarse", "feature_coarse", "depth_coarse", "weights_fine", "feature_fine", "feature_fine_random", "depth_fine"]


@torch.no_grad()
@pytest.mark.parametrize("precision", PRECISIONS + ["bf16_fc"])
def test_mirror_returns_the_lean_key_set_with_the_full_values(scene, precision):
    """bf16 / f16: the new kernels.  bf16_fc: its own two-launch path is untouched -- it renders as without the flag and drops keys."""
    from crnerf_amd.models.rendering import render_rays_cross_ray
    args, models, emb, rays, _ = scene
    call = lambda **kw: render_rays_cross_ray(models, emb, rays[:40], None, 64, False, 0, 0, 128, 4096, False, test_time=True, args=args,  # noqa: E731
                                              precision=precision, **kw)
    full, lean = call(), call(lean=True)
    assert list(full) == FULL_KEYS and list(lean) == LEAN_KEYS
    assert lean["feature_fine_random"] is lean["feature_fine"]
    assert bool(torch.isfinite(full["feature_fine"]).all())
    for k in LEAN_KEYS:
        assert torch.equal(lean[k], full[k]), k


@torch.no_grad()
@pytest.mark.parametrize("precision", PRECISIONS)
def test_batched_inference_and_decode_give_the_same_image(scene, precision):
    args, models, emb, rays, style = scene
    H, W = 12, 16
    run = lambda **kw: pipeline.batched_inference(models, emb, rays, None, 64, 128, False, 100, False, args=args, precision=precision, **kw)  # noqa: E731
    full, lean = run(), run(lean=True)                  # 192 rays in chunks of 100: two ray chunks
    assert list(lean) == LEAN_KEYS and lean["feature_fine"].shape == (H * W, 64)
    img_full = pipeline.decode_image(models, full, H, W, style)
    img_lean = pipeline.decode_image(models, lean, H, W, style)
    assert img_lean.shape == (H * W, 3) and torch.equal(img_lean, img_full)

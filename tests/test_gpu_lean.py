"""The lean inference render (crnerf_render_rays_lean_f32; ops.render_rays(..., lean=True); render_rays_cross_ray(..., lean=True)).

The lean kernel is the full fp32 kernel minus work nobody reads: its coarse tiles stop behind the sigma head (the weight ring walks 124 of the 151
stages there), no coarse feature is composited, nothing of the coarse pass and no weights_fine reach HBM.  The trunk, the sigma head, the
compositing scan, sample_pdf, the merge and the fine pass execute the full kernel's instructions in the full kernel's order, so feature_fine,
depth_fine and z_fine are compared with torch.equal -- a property by construction, not a tolerance.  Every shape is one way the ring or the quad
logic could go wrong (see CASES)."""
import ctypes

import numpy as np
import pytest
import torch

import crnerf_amd.synth as synth
from crnerf_amd import _lib, ops, pipeline
from oracle import cpu_ref as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ST_C, ST_F = synth.mlp_state(5, 3.0, 1.0), synth.mlp_state(6, 3.0, 1.0)      # the parity tests' scaling (gain 3, sigma bias 1)


def C(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@pytest.fixture(scope="module")
def packs():
    pk = lambda st: ops.pack_mlp_weights({k: C(v) for k, v in st.items()})  # noqa: E731
    return pk(ST_C), pk(ST_F)


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
    "dynamic_sched_1030x64+128": (1030, 64, 128, False, False),   # 258 quads on 256 CUs: the device-side quad counter; 124 / 151 alternation across quads
    "one_walk_8x3+5_disp": (8, 3, 5, True, False),                # one coarse walk per ray, partial last steps in both passes
    "one_walk_8x33+31_disp": (8, 33, 31, True, False),
    "maximum_8x256+256": (8, 256, 256, False, False),             # 8 short walks then 16 long ones
    "tensors_64x48+40": (64, 48, 40, False, True),                # view_dir, noise tensors, noise_std = 1, caller's z_coarse, per-ray u
}
_REF = {}


def _both(packs, name):
    """(inputs, full render, lean render) of a case; rendered once and shared, never modified."""
    if name not in _REF:
        R, nc, ni, disp, rich = CASES[name]
        rays, kw = _inputs(R, nc, ni, disp, rich)
        with torch.no_grad():
            full = ops.render_rays(packs[0], packs[1], rays, nc, ni, **kw)
            lean = ops.render_rays(packs[0], packs[1], rays, nc, ni, lean=True, **kw)
        torch.cuda.synchronize()
        _REF[name] = (rays, kw, full, lean)
    return _REF[name]


@pytest.mark.parametrize("name", list(CASES))
def test_lean_equals_full_bit_for_bit(packs, name):
    _, _, full, lean = _both(packs, name)
    assert sorted(lean) == ["depth_fine", "feature_fine", "z_fine"]
    assert bool(torch.isfinite(full["feature_fine"]).all())
    for k in ("z_fine", "depth_fine", "feature_fine"):
        assert torch.equal(lean[k], full[k]), "%s: %s differs in %d places, max|d| %g" % (
            name, k, int((lean[k] != full[k]).sum()), float((lean[k] - full[k]).abs().max()))


def test_back_to_back_lean_launches_leave_the_scheduler_words_zeroed(packs):
    """Two lean launches and a full one on the same stream, nothing in between: every one of them takes the dynamic quad counter from zero."""
    name = "dynamic_sched_1030x64+128"
    rays, kw, full, _ = _both(packs, name)
    R, nc, ni = CASES[name][:3]
    with torch.no_grad():
        a = ops.render_rays(packs[0], packs[1], rays, nc, ni, lean=True, **kw)
        b = ops.render_rays(packs[0], packs[1], rays, nc, ni, lean=True, **kw)
        c = ops.render_rays(packs[0], packs[1], rays, nc, ni, **kw)
    torch.cuda.synchronize()
    for k in ("z_fine", "depth_fine", "feature_fine"):
        assert torch.equal(a[k], full[k]) and torch.equal(b[k], full[k]), k
    for k in full:
        assert torch.equal(c[k], full[k]), k


def test_lean_against_the_oracle(packs):
    """The R = 64 case (view_dir, noise, caller's depths, per-ray u) against oracle.cpu_ref at the kernel's own fine depths, with the bars of
    tests/test_gpu_parity.py's fused-render comparison (feature 1e-5, depth 2e-5)."""
    rays, kw, _, lean = _both(packs, "tensors_64x48+40")
    r, zf = rays.cpu(), lean["z_fine"].cpu()
    assert bool((zf[:, 1:] >= zf[:, :-1]).all())
    raw = O._run_model(O.to_torch(ST_F), r, zf, O.posenc(kw["view_dir"].cpu(), 4), 32768)
    _, f2, d2 = O.composite(raw, zf, kw["noise_fine"].cpu(), 1.0)
    torch.testing.assert_close(lean["feature_fine"].cpu(), f2, atol=1e-5, rtol=0)
    torch.testing.assert_close(lean["depth_fine"].cpu(), d2, atol=2e-5, rtol=0)


def _args(packs, rays, nc, ni, out):
    a = _lib.RenderArgs()
    a.packed_coarse, a.packed_fine, a.rays = packs[0].data_ptr(), packs[1].data_ptr(), rays.data_ptr()
    a.n_rays, a.n_samples, a.n_importance = rays.shape[0], nc, ni
    a.feature_fine, a.depth_fine = out["feature_fine"].data_ptr(), out["depth_fine"].data_ptr()
    return a


def test_entry_point_validation(packs):
    lib = _lib.load()
    rays, _, full, _ = _both(packs, "ragged_quad_5x64+128")
    out = {"feature_fine": torch.zeros(5, 64, device=DEV), "depth_fine": torch.zeros(5, device=DEV), "z_coarse_used": torch.zeros(5, 64, device=DEV)}
    call = lambda a: lib.crnerf_render_rays_lean_f32(ctypes.byref(a), _lib.stream_ptr())  # noqa: E731
    a = _args(packs, rays, 64, 0, out)
    assert call(a) in (-2, -3)                                   # n_importance = 0: CRNERF_ERR_SHAPE (a config error would do)
    a = _args(packs, rays, 64, 128, out)
    a.rng_flags = 1
    assert call(a) == -3                                         # CRNERF_ERR_CONFIG
    a = _args(packs, rays, 64, 128, out)
    a.z_coarse_out = out["z_coarse_used"].data_ptr()
    assert call(a) == -3
    a = _args(packs, rays, 64, 128, out)
    a.packed_fine = None
    assert call(a) == -1
    torch.cuda.synchronize()
    assert float(out["feature_fine"].abs().max()) == 0.0         # a refused call launched nothing
    # NULL coarse outputs / weights_fine / z_fine / z_steps / u are accepted; in-kernel linspace tables in both kernels
    a = _args(packs, rays, 64, 128, out)
    assert call(a) == 0
    ref = ops.render_rays(packs[0], packs[1], rays, 64, 128)
    torch.cuda.synchronize()
    assert torch.equal(out["feature_fine"], ref["feature_fine"]) and torch.equal(out["depth_fine"], ref["depth_fine"])
    with pytest.raises(ValueError):
        ops.render_rays(packs[0], packs[1], rays, 64, 128, lean=True, train=True)
    with pytest.raises(ValueError):
        ops.render_rays(packs[0], packs[1], rays, 64, 128, lean=True, rng={"seed": 1, "jitter": True})


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
@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_mirror_returns_the_lean_key_set_with_the_full_values(scene, precision):
    from crnerf_amd.models.rendering import render_rays_cross_ray
    args, models, emb, rays, _ = scene
    call = lambda **kw: render_rays_cross_ray(models, emb, rays[:40], None, 64, False, 0, 0, 128, 4096, False, test_time=True, args=args,  # noqa: E731
                                              precision=precision, **kw)
    full, lean = call(), call(lean=True)
    assert list(full) == FULL_KEYS and list(lean) == LEAN_KEYS
    assert lean["feature_fine_random"] is lean["feature_fine"]
    for k in LEAN_KEYS:
        assert torch.equal(lean[k], full[k]), k
    noran = call(lean=True, output_random=False)
    assert list(noran) == ["feature_fine", "depth_fine"]
    # perturb > 0 at inference: the draws are torch's, handed to the kernel as tensors -- same seed, same image
    if precision == "f32":
        pert = lambda **kw: render_rays_cross_ray(models, emb, rays[:40], None, 64, False, 1.0, 0, 128, 4096, False, args=args, **kw)  # noqa: E731
        torch.manual_seed(7)
        pf = pert()
        torch.manual_seed(7)
        pl = pert(lean=True)
        assert list(pl) == LEAN_KEYS and torch.equal(pl["feature_fine"], pf["feature_fine"]) and torch.equal(pl["depth_fine"], pf["depth_fine"])
        assert not torch.equal(pf["feature_fine"], full["feature_fine"])


def test_mirror_without_fine_pass_and_in_grad_mode(scene):
    from crnerf_amd.models.rendering import render_rays_cross_ray
    args, models, emb, rays, _ = scene
    with torch.no_grad():
        res = render_rays_cross_ray({"coarse": models["coarse"]}, emb, rays[:8], None, 64, False, 0, 0, 0, 4096, False, args=args, lean=True)
    assert list(res) == ["weights_coarse", "feature_coarse", "depth_coarse"]           # N_importance = 0: the flag means nothing
    with pytest.raises(ValueError):
        render_rays_cross_ray(models, emb, rays[:8], None, 64, False, 0, 0, 128, 4096, False, args=args, lean=True)


def test_batched_inference_and_decode_give_the_same_image(scene):
    args, models, emb, rays, style = scene
    H, W = 12, 16
    run = lambda **kw: pipeline.batched_inference(models, emb, rays, None, 64, 128, False, 100, False, args=args, **kw)  # noqa: E731
    full, lean = run(), run(lean=True)                  # 192 rays in chunks of 100: two ray chunks
    assert list(lean) == LEAN_KEYS and lean["feature_fine"].shape == (H * W, 64)
    img_full = pipeline.decode_image(models, full, H, W, style)
    img_lean = pipeline.decode_image(models, lean, H, W, style)
    assert img_lean.shape == (H * W, 3) and torch.equal(img_lean, img_full)

"""lean=True in the composite precisions "bf16_hc" and "bf16_fc": the coarse-weights renders (crnerf_render_coarse_weights_f32h2 / _f32x3 /
_f32x3_repair / _f16; ops.render_coarse_weights) and the fine launch without weights_fine (crnerf_render_rays_lean_bf16_fine;
ops.render_rays_bf16_fine(..., lean=True)), include/crnerf_lean_composite.h.

A coarse-weights kernel is the full coarse-only kernel minus work nobody reads: every tile walks layers 1..8 and static_sigma (the weight ring runs
the shorter pass), alpha, the transmittance scan and the weights execute the full kernel's arithmetic in its order, and nothing but weights_coarse
is stored.  The lean fine kernel is the fine-only kernel minus one store.  So every comparison against the full launches is torch.equal -- a
property by construction, not a tolerance.  Every shape is one way the shorter walk, the ring phase or the quad logic could go wrong (see the
CASES tables)."""
import numpy as np
import pytest
import torch

import crnerf_amd.synth as synth
from crnerf_amd import ops, pipeline
from oracle import cpu_ref as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ST_C, ST_F = synth.mlp_state(5, 3.0, 1.0), synth.mlp_state(6, 3.0, 1.0)      # tests/test_gpu_lean_pair.py's states; largest |weight| 1.2
MARK = 0x7fc00000


def C(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


_PACKS = {}


def pack(state_id, precision):
    """The pack of ST_C ("c") / ST_F ("f") for a precision; packed once."""
    if (state_id, precision) not in _PACKS:
        st = ST_C if state_id == "c" else ST_F
        _PACKS[(state_id, precision)] = ops.pack_mlp_weights({k: C(v) for k, v in st.items()}, precision=precision)
    return _PACKS[(state_id, precision)]


def _coarse_inputs(R, nc, disp, rich):
    """(rays, what both calls take, what only the full call takes)."""
    rays = synth.rays(R, seed=3)
    kw, full_only = dict(use_disp=disp, z_steps=torch.linspace(0, 1, nc).to(DEV)), {}
    if rich:       # the caller's coarse depths, density noise with noise_std = 1, and a view direction -- which the trunk never reads
        rng = np.random.default_rng(4)
        vd = rng.normal(size=(R, 3)).astype(np.float32)
        vd /= np.linalg.norm(vd, axis=-1, keepdims=True)
        kw = dict(use_disp=disp, z_coarse=C(np.sort(rng.uniform(rays[:, 6:7], rays[:, 7:8], (R, nc)).astype(np.float32), -1)),
                  noise_coarse=C(rng.normal(size=(R, nc)).astype(np.float32)), noise_std=1.0)
        full_only = dict(view_dir=C(vd))
    return C(rays), kw, full_only


COARSE_CASES = {
    "ragged_quad_5x64": (5, 64, False, False),                # a ragged last ray quad
    "second_round_1030x64": (1030, 64, False, False),         # 258 quads on 256 CUs: a second persistent round / the device-side quad counter
    "partial_tile_8x3_disp": (8, 3, True, False),             # one partial tile
    "second_tile_one_sample_8x33": (8, 33, False, False),     # the second tile holds one sample
    "maximum_8x256": (8, 256, False, False),                  # the maximum sample count
    "tensors_64x48": (64, 48, False, True),                   # caller's z_coarse, noise_coarse, noise_std = 1; view_dir must not matter
    # pair core only: two and three 64-sample steps, i.e. trunk walks in both ring phases within a ray and an odd number of them per ray
    "ring_phase_8x96": (8, 96, False, False),
    "ring_phase_8x160": (8, 160, False, False),
}
COARSE_PARAMS = [(p, n) for p in ("f32h2", "f32x3", "f16") for n in COARSE_CASES if p == "f16" or not n.startswith("ring_phase")]


@torch.no_grad()
@pytest.mark.parametrize("precision,name", COARSE_PARAMS)
def test_coarse_weights_equal_the_full_coarse_only_render_bit_for_bit(precision, name):
    R, nc, disp, rich = COARSE_CASES[name]
    rays, kw, full_only = _coarse_inputs(R, nc, disp, rich)
    pk = pack("c", precision)
    full = ops.render_rays(pk, None, rays, nc, 0, precision=precision, **kw, **full_only)["weights_coarse"]
    got = ops.render_coarse_weights(pk, rays, nc, precision=precision, **kw)
    torch.cuda.synchronize()
    assert list(got) == ["weights_coarse"] and got["weights_coarse"].shape == (R, nc)
    got = got["weights_coarse"]
    assert bool(torch.isfinite(full).all()) and float(full.sum()) > 0
    assert torch.equal(got, full), "%s %s: %d of %d weights differ, max|d| %g" % (
        precision, name, int((got != full).sum()), got.numel(), float((got - full).abs().max()))


# ---------------------------------------------------------------- the fine launch
FINE_CASES = {
    "ragged_quad_5x64+128": (5, 64, 128, False, False),
    "second_round_1030x64+128": (1030, 64, 128, False, False),
    "one_step_8x33+31_disp": (8, 33, 31, True, False),
    "odd_steps_8x160+96": (8, 160, 96, False, False),
    "maximum_8x256+256": (8, 256, 256, False, False),
    "tensors_64x48+40": (64, 48, 40, False, True),            # view_dir, per-ray u, noise_fine with noise_std = 1
}
_FINE = {}


def _fine_both(name):
    """(inputs, full fine launch, lean fine launch) of a case on the x3 core's coarse weights; rendered once and shared, never modified."""
    if name not in _FINE:
        R, nc, ni, disp, rich = FINE_CASES[name]
        rays = C(synth.rays(R, seed=3))
        kw = dict(use_disp=disp, z_steps=torch.linspace(0, 1, nc).to(DEV), u=torch.linspace(0, 1, ni).to(DEV), want_z_fine=True)
        if rich:
            rng = np.random.default_rng(4)
            vd = rng.normal(size=(R, 3)).astype(np.float32)
            vd /= np.linalg.norm(vd, axis=-1, keepdims=True)
            kw.update(view_dir=C(vd), u=C(rng.uniform(0, 1, (R, ni)).astype(np.float32)),
                      noise_fine=C(rng.normal(size=(R, nc + ni)).astype(np.float32)), noise_std=1.0)
        with torch.no_grad():
            wc = ops.render_coarse_weights(pack("c", "f32x3"), rays, nc, precision="f32x3", use_disp=disp, z_steps=kw["z_steps"])["weights_coarse"]
            full = ops.render_rays_bf16_fine(pack("f", "bf16"), rays, wc, nc, ni, **kw)
            lean = ops.render_rays_bf16_fine(pack("f", "bf16"), rays, wc, nc, ni, lean=True, **kw)
        torch.cuda.synchronize()
        _FINE[name] = (rays, wc, kw, full, lean)
    return _FINE[name]


@pytest.mark.parametrize("name", list(FINE_CASES))
def test_lean_fine_launch_equals_the_full_one(name):
    _, _, _, full, lean = _fine_both(name)
    assert sorted(full) == ["depth_fine", "feature_fine", "weights_fine", "z_fine"]
    assert sorted(lean) == ["depth_fine", "feature_fine", "z_fine"]              # no weights_fine key: it is neither allocated nor written
    assert bool(torch.isfinite(full["feature_fine"]).all())
    for k in ("z_fine", "depth_fine", "feature_fine"):
        assert torch.equal(lean[k], full[k]), "%s: %s differs in %d places" % (name, k, int((lean[k] != full[k]).sum()))


@torch.no_grad()
def test_back_to_back_launches_on_one_stream():
    """The fp16 coarse-weights launch, the lean fine launch and a full bf16 render, twice, nothing in between: each equals its solo result, so every
    launch took the pair core's dynamic quad counter (1,030 rays: 258 quads on 256 workgroups) from zero -- the words came back zeroed each time."""
    name = "second_round_1030x64+128"
    rays, wc, kw, full, _ = _fine_both(name)
    R, nc, ni = FINE_CASES[name][:3]
    ckw = dict(z_steps=kw["z_steps"])
    solo_c = ops.render_coarse_weights(pack("c", "f16"), rays, nc, precision="f16", **ckw)["weights_coarse"]
    torch.cuda.synchronize()
    solo_b = ops.render_rays(pack("c", "bf16"), pack("f", "bf16"), rays, nc, ni, precision="bf16", **kw)
    torch.cuda.synchronize()
    runs = []
    for _ in range(2):
        a = ops.render_coarse_weights(pack("c", "f16"), rays, nc, precision="f16", **ckw)["weights_coarse"]
        b = ops.render_rays_bf16_fine(pack("f", "bf16"), rays, wc, nc, ni, lean=True, **kw)
        c = ops.render_rays(pack("c", "bf16"), pack("f", "bf16"), rays, nc, ni, precision="bf16", **kw)
        runs.append((a, b, c))
    torch.cuda.synchronize()
    for a, b, c in runs:
        assert torch.equal(a, solo_c)
        for k in ("z_fine", "depth_fine", "feature_fine"):
            assert torch.equal(b[k], full[k]), k
        for k in solo_b:
            assert torch.equal(c[k], solo_b[k]), k


# ---------------------------------------------------------------- the mark and its repair
def _overflow_case():
    """tests/test_gpu_h2.py's overflow net with one more amplifying layer: hidden unit 0 of xyz_encoding_1 / _2 / _3 multiplies the raw x coordinate
    by 250 * 250 * 4, so h2 and h3 -- operands of layers 3 and 4 -- pass 65,504 where x is of ordinary size; every weight packs for the h2 core
    (|w| < 255) and for fp16.  192 of the 256 rays have tiny origins and depths and stay in range.  Returns the state, the rays and, from the trunk
    in float64 on the CPU, which rays leave fp16's range for certain (a sample 3 % beyond the limit) and which stay inside for certain (every
    sample 3 % below); with or without h8, which the fp16 pair core converts and the h2 core does not."""
    import torch.nn.functional as F
    nc = 64
    st = dict(synth.mlp_state(5, 1.0))
    for layer, gain in ((1, 250.0), (2, 250.0), (3, 4.0)):
        w = st["xyz_encoding_%d.0.weight" % layer].copy()
        w[0, 0] = gain
        st["xyz_encoding_%d.0.weight" % layer] = w
    rays = synth.rays(256, seed=3, H=16, W=16).copy()
    rays[:192, 0:3] *= 1e-3
    rays[:192, 6] = 1e-4
    rays[:192, 7] = 2e-3
    r, zt = torch.from_numpy(rays), torch.linspace(0, 1, nc)
    z = r[:, 6:7] * (1 - zt) + r[:, 7:8] * zt
    x = O.posenc((r[:, None, 0:3] + r[:, None, 3:6] * z[..., None]).reshape(-1, 3), 15).double()
    w = {k: torch.from_numpy(v).double() for k, v in st.items()}
    worst7 = worst8 = x.abs().max(1).values
    h = x
    for layer in range(1, 9):
        if layer == 5:
            h = torch.cat((x, h), 1)
        h = F.relu(F.linear(h, w["xyz_encoding_%d.0.weight" % layer], w["xyz_encoding_%d.0.bias" % layer]))
        worst8 = torch.maximum(worst8, h.max(1).values)
        if layer < 8:
            worst7 = worst8
    over, under = [], []
    for worst in (worst7, worst8):
        t = worst.view(-1, nc) / 65504.0
        over.append((t >= 1.03).any(1))
        under.append((t <= 0.97).all(1))
    assert torch.equal(over[0], over[1]) and torch.equal(under[0], under[1])
    assert int(over[0].sum()) >= 8 and int(under[0][192:].sum()) >= 8 and bool(under[0][:192].all())
    return st, C(rays), nc, over[0], under[0]


def _marked(w):
    return (w[:, 0].view(torch.int32) == MARK).cpu()


@torch.no_grad()
def test_mark_and_repair():
    st, rays, nc, over, under = _overflow_case()
    dev = {k: C(v) for k, v in st.items()}
    zs = torch.linspace(0, 1, nc, device=DEV)
    auto = ops.pack_mlp_weights(dev, precision="auto")
    assert auto.h2 is not None
    f16 = ops.pack_mlp_weights(dev, precision="f16")
    x3 = ops.render_coarse_weights(auto.x3, rays, nc, precision="f32x3", z_steps=zs)["weights_coarse"]
    assert bool(torch.isfinite(x3).all())
    runs = {"f32h2": (ops.render_coarse_weights(auto.h2, rays, nc, precision="f32h2", z_steps=zs)["weights_coarse"],
                      ops.render_coarse_weights(auto, rays, nc, precision="auto", z_steps=zs)["weights_coarse"]),
            "f16": (ops.render_coarse_weights(f16, rays, nc, precision="f16", z_steps=zs)["weights_coarse"],
                    ops.render_coarse_weights(f16, rays, nc, precision="f16", z_steps=zs, repair_x3=auto.x3)["weights_coarse"])}
    torch.cuda.synchronize()
    for name, (marked, repaired) in runs.items():
        m = _marked(marked)
        print("%s: %d rays marked; %d leave fp16's range for certain, %d stay inside for certain" % (name, int(m.sum()), int(over.sum()), int(under.sum())))
        assert bool(m[over].all()) and not bool(m[under].any()), name                 # exactly those rays
        assert torch.equal(m, torch.isnan(marked[:, 0]).cpu()), name                  # the mark is the only NaN a row can start with
        assert bool(torch.isfinite(marked[~m.to(DEV)]).all()), name
        quad = m.view(-1, 4).any(1)[:, None].expand(-1, 4).reshape(-1).to(DEV)
        assert not bool(torch.isnan(repaired).any()), name
        assert torch.equal(repaired[quad], x3[quad]), name                             # the marked quads' rows: the x3 core's
        assert torch.equal(repaired[~quad], marked[~quad]), name                       # every other row: unchanged
    # a pack that carries the range flag marks every ray, and the repair renders all of them
    big = dict(st)
    wbig = big["xyz_encoding_4.0.weight"].copy()
    wbig[7, 9] = 300.0
    big["xyz_encoding_4.0.weight"] = wbig
    devb = {k: C(v) for k, v in big.items()}
    h2_flagged = ops.pack_mlp_weights_auto(devb, check=False)
    wf = ops.render_coarse_weights(h2_flagged.h2, rays[:10], nc, precision="f32h2", z_steps=zs)["weights_coarse"]
    assert bool(_marked(wf).all())
    wr = ops.render_coarse_weights(h2_flagged, rays[:10], nc, precision="auto", z_steps=zs)["weights_coarse"]
    assert torch.equal(wr, ops.render_coarse_weights(h2_flagged.x3, rays[:10], nc, precision="f32x3", z_steps=zs)["weights_coarse"])


# ---------------------------------------------------------------- through the mirror
class _Args:
    nerf_out_dim, img_wh, pertubeCord = 64, [24, 20], False
    N_samples, N_importance, use_disp = 64, 128, False


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
    style = C(np.random.default_rng(1).uniform(0, 1, (1, 64, 32, 32)).astype(np.float32))
    return args, models, emb, style


MODES = ["bf16_hc", "bf16_fc"]
LEAN_KEYS = ["feature_fine", "feature_fine_random", "depth_fine"]
FULL_KEYS = ["weights_coarse", "feature_coarse", "depth_coarse", "weights_fine", "feature_fine", "feature_fine_random", "depth_fine"]


@torch.no_grad()
@pytest.mark.parametrize("mode", MODES)
def test_mirror_takes_the_lean_launches_and_returns_the_full_values(scene, mode, monkeypatch):
    """The test that fails without the feature: on the parent the composite modes render as without the flag and drop keys, and
    ops.render_coarse_weights does not exist."""
    from crnerf_amd.models.rendering import render_rays_cross_ray
    args, models, emb, _ = scene
    calls = []
    real = ops.render_coarse_weights

    def spy(*a, **kw):
        calls.append(kw.get("precision"))
        return real(*a, **kw)
    monkeypatch.setattr(ops, "render_coarse_weights", spy)
    rays = C(synth.rays(40, seed=5, H=5, W=8))
    call = lambda **kw: render_rays_cross_ray(models, emb, rays, None, 64, False, 0, 0, 128, 4096, False, test_time=True, args=args,  # noqa: E731
                                              precision=mode, **kw)
    full = call()
    assert calls == [] and list(full) == FULL_KEYS
    lean = call(lean=True)
    assert calls == ["auto" if mode == "bf16_hc" else "f16"]                    # one coarse-weights launch (+ its repair) per call
    assert list(lean) == LEAN_KEYS and lean["feature_fine_random"] is lean["feature_fine"]
    assert bool(torch.isfinite(full["feature_fine"]).all())
    for k in LEAN_KEYS:
        assert torch.equal(lean[k], full[k]), k


@torch.no_grad()
@pytest.mark.parametrize("mode", MODES)
def test_render_frame_gives_the_same_bytes(scene, mode):
    args, models, emb, style = scene
    W, H = args.img_wh
    focal = W / 2 / np.tan(np.pi / 6)
    K = np.array([[focal, 0, W / 2], [0, focal, H / 2], [0, 0, 1]])
    c2w = np.array([[1, 0, 0, 0.05], [0, -1, 0, 0.02], [0, 0, -1, 0.1]], dtype=np.float32)
    run = lambda **kw: pipeline.render_frame(models, emb, None, style, H, W, K, c2w, args, chunk=200, precision=mode, a_emb=style, **kw)  # noqa: E731
    full, lean = run(), run(lean=True)                  # 480 rays in chunks of 200: three ray chunks, the last ragged
    assert full.shape == (H, W, 3) and bool(torch.isfinite(full).all())
    assert torch.equal(lean, full)


@torch.no_grad()
@pytest.mark.parametrize("mode", MODES)
def test_lean_call_allocates_less(scene, mode):
    """A condition, not a measurement.  By the tensor list the ordinary call allocates 4 R (64 + 1 + Nc + Ni) bytes more than the lean one
    (feature_coarse, depth_coarse, weights_fine), all of it live at the call's peak; the bar is the weights_fine part alone."""
    from crnerf_amd.models.rendering import render_rays_cross_ray
    args, models, emb, _ = scene
    R, nc, ni = 4096, 64, 128
    rays = C(synth.rays(R, seed=0, H=64, W=64))
    call = lambda **kw: render_rays_cross_ray(models, emb, rays, None, nc, False, 0, 0, ni, 32768, False, test_time=True, args=args,  # noqa: E731
                                              precision=mode, **kw)
    peaks = {}
    for lean in (False, True):
        call(lean=lean)                                 # packs and linspace tables are cached by the first call
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        out = call(lean=lean)
        torch.cuda.synchronize()
        peaks[lean] = torch.cuda.max_memory_allocated() - base
        del out
    print("%s: peak of the ordinary call %d bytes, of the lean call %d bytes" % (mode, peaks[False], peaks[True]))
    assert peaks[False] - peaks[True] >= 4 * R * (nc + ni)

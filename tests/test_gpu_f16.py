"""GPU parity of the fp16-operand variants (crnerf_mlp_forward_f16 / crnerf_render_rays_f16) and of precision="bf16_fc".

Reference: oracle/cpu_ref.mlp_forward_bf16 / render_rays(precision="bf16") with its operand rounding replaced by fp16 rounding (`f16_emulation`).
Products of two fp16 values are exact in fp32, so -- as for bf16 -- the kernel differs from the emulation by summation order (and the fast sigmoid /
softplus) only; the bars are therefore the ones tests/test_gpu_bf16.py holds the bf16 core to against its emulation, unchanged.
fp16 subnormals: the gfx950 MFMA keeps subnormal fp16 inputs and v_cvt_pk_f16_f32 produces them (test_subnormal_weights_are_kept measures it
through crnerf_mlp_forward_f16), so the emulation keeps them too: torch's fp32 -> fp16 conversion does.
"""
import contextlib

import numpy as np
import pytest
import torch

import crnerf_amd.synth as synth
from crnerf_amd import ops, pipeline
from oracle import cpu_ref as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F16_MAX = 65504.0
F16_OVERFLOW = 65520.0          # the smallest magnitude that rounds (RNE) to inf


def C(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def f16_round(t):
    return t.to(torch.float16).to(torch.float32)


def f16_round_flushed(t):
    r = f16_round(t)
    return torch.where(r.abs() < 2.0 ** -14, torch.zeros_like(r), r)


@contextlib.contextmanager
def f16_emulation(round_fn=f16_round):
    """oracle.cpu_ref's bf16 restatement with fp16 operand rounding."""
    keep = O.bf16_round
    O.bf16_round = round_fn
    try:
        yield
    finally:
        O.bf16_round = keep


def emu_mlp(w, x, sigma_only=False, round_fn=f16_round):
    with f16_emulation(round_fn):
        return O.mlp_forward_bf16(w, x, sigma_only=sigma_only)


def emu_render(wc, wf, rays, nc, ni, **kw):
    with f16_emulation():
        return O.render_rays(wc, wf, rays, nc, ni, precision="bf16", **kw)


def packed(state, precision="f16"):
    return ops.pack_mlp_weights({k: C(v) for k, v in state.items()}, precision=precision)


def embedded(n, seed):
    g = torch.Generator().manual_seed(seed)
    pts = torch.rand(n, 3, generator=g) * 6 - 3
    dirs = torch.nn.functional.normalize(torch.randn(n, 3, generator=g), dim=1)
    return torch.cat((O.posenc(pts, 15), O.posenc(dirs, 4)), 1)


def err(got, want):
    d = (got.detach().double().cpu() - torch.as_tensor(want).double()).abs()
    return float(d.max()), float(d.mean())


def coarse_state(g):
    return {k[len("sd__nerf_coarse."):]: np.ascontiguousarray(v) for k, v in g.items() if k.startswith("sd__nerf_coarse.")}


# ------------------------------------------------------------------ 1. the MLP against the fp16 emulation
@torch.no_grad()
@pytest.mark.parametrize("n", [1, 31, 64, 65, 255, 256, 257, 1000])
def test_mlp_f16_ragged_sizes_vs_f16_emulation(n):
    st = synth.mlp_state(7, 1.0)
    x = embedded(n, n)
    got = ops.mlp_forward(packed(st), x.to(DEV), precision="f16")
    want = emu_mlp(O.to_torch(st), x)
    assert got.shape == (n, 65)
    mx, mean = err(got, want)
    print("f16 mlp n=%d: max %.3e mean %.3e" % (n, mx, mean))
    assert mx < 1e-3 and mean < 2e-6, (mx, mean)            # tests/test_gpu_bf16.py's bars for the same kind of difference


@torch.no_grad()
def test_mlp_f16_peaky_weights_and_sigma_only():
    st = synth.mlp_state(7, 3.0)
    x = embedded(1000, 3)
    got = ops.mlp_forward(packed(st), x.to(DEV), precision="f16")
    want = emu_mlp(O.to_torch(st), x)
    mx, mean = err(got[:, :64], want[:, :64])
    print("f16 mlp peaky: max %.3e mean %.3e" % (mx, mean))
    assert mx < 0.1 and mean < 2e-4, (mx, mean)
    rel = float(((got[:, 64].cpu() - want[:, 64]).abs() / (want[:, 64].abs() + 1)).max())
    assert rel < 2e-2, rel
    so = ops.mlp_forward(packed(st), x[:, :93].contiguous().to(DEV), sigma_only=True, precision="f16")
    assert so.shape == (1000, 1)
    assert torch.equal(so[:, 0], got[:, 64])
    mx_s, _ = err(so, emu_mlp(O.to_torch(st), x[:, :93].contiguous(), sigma_only=True))
    assert mx_s / (float(want[:, 64].abs().max()) + 1) < 2e-2, mx_s


@torch.no_grad()
@pytest.mark.parametrize("fixture", ["g2_mlp", "g15_trained", "g16_trained"])
def test_mlp_f16_golden_and_trained_coarse_weights(golden, fixture):
    g = golden(fixture)
    if fixture == "g2_mlp":
        st, x = synth.mlp_state(int(g["seed_default"]), float(g["gain_default"])), torch.from_numpy(np.ascontiguousarray(g["x"]))
    else:
        st = coarse_state(g)
        rays = torch.from_numpy(np.ascontiguousarray(g["rays"]))[:48]
        z = torch.linspace(0, 1, 64)[None, :] * (rays[:, 7:8] - rays[:, 6:7]) + rays[:, 6:7]
        pts = (rays[:, None, 0:3] + rays[:, None, 3:6] * z[..., None]).reshape(-1, 3)
        x = torch.cat((O.posenc(pts, 15), O.posenc(rays[:, 3:6], 4).repeat_interleave(64, 0)), 1)[:3001].contiguous()   # ragged: 3001 = 11 x 256 + 185
    w = O.to_torch(st)
    got = ops.mlp_forward(packed(st), x.to(DEV), precision="f16")
    want = emu_mlp(w, x)
    mx, mean = err(got[:, :64], want[:, :64])
    rel = float(((got[:, 64].cpu() - want[:, 64]).abs() / (want[:, 64].abs() + 1)).max())
    print("f16 mlp %s: features max %.3e mean %.3e, sigma rel %.3e" % (fixture, mx, mean, rel))
    assert mx < 1e-3 and mean < 2e-6 and rel < 1e-3, (mx, mean, rel)
    so = ops.mlp_forward(packed(st), x[:, :93].contiguous().to(DEV), sigma_only=True, precision="f16")
    assert torch.equal(so[:, 0], got[:, 64])
    # 11 significand bits instead of 8: closer to the fp32 forward than the bf16 core is
    f32 = O.mlp_forward(w, x)
    bf = ops.mlp_forward(packed(st, "bf16"), x.to(DEV), precision="bf16")
    assert err(got[:, :64], f32[:, :64])[1] < 0.5 * err(bf[:, :64], f32[:, :64])[1]


# ------------------------------------------------------------------ 2. the fused renderer against the emulated render
@torch.no_grad()
@pytest.mark.parametrize("nc,ni,disp", [(64, 128, False), (64, 0, False), (64, 128, True), (48, 40, False), (256, 256, False), (3, 5, False)])
def test_render_f16_vs_f16_emulation_at_identical_depths(nc, ni, disp):
    R = 96
    rays_np = synth.rays(R, seed=5)
    st_c, st_f = synth.mlp_state(21, 2.0), synth.mlp_state(22, 2.0)
    zt = torch.linspace(0, 1, nc)
    ut = torch.linspace(0, 1, ni) if ni else None
    out = ops.render_rays(packed(st_c), packed(st_f) if ni else None, C(rays_np), nc, ni, use_disp=disp, z_steps=zt.to(DEV),
                          u=ut.to(DEV) if ni else None, want_z_fine=bool(ni), precision="f16")
    orc = emu_render(O.to_torch(st_c), O.to_torch(st_f), torch.from_numpy(rays_np), nc, ni, use_disp=disp, z_steps=zt,
                     z_fine=out["z_fine"].cpu() if ni else None)
    keys = ["weights_coarse", "feature_coarse", "depth_coarse"] + (["weights_fine", "feature_fine", "depth_fine"] if ni else [])
    for k in keys:
        mx, mean = err(out[k], orc[k])
        print("f16 render %d+%d %s: max %.3e mean %.3e" % (nc, ni, k, mx, mean))
        assert mx < 2e-2 and mean < 2e-4, (k, mx, mean)      # the bf16 render test's bars
    if ni:
        z = out["z_fine"]
        assert bool((z[:, 1:] >= z[:, :-1]).all())
        assert float(out["weights_fine"].sum(-1).max()) <= 1 + 1e-5


# ------------------------------------------------------------------ 3. the pack
@torch.no_grad()
def test_f16_pack_fragment_permutation_by_one_hot_inputs():
    """A one-hot input column reproduces that column of W1 (+ bias) through layer 1: catches any row / column / slot permutation of the fragment
    stream (tests/test_gpu_parity.py does the same for the fp32 pack).  Tolerance: the emulation's own summation-order noise."""
    st = synth.mlp_state(3, 1.0)
    x = torch.zeros(120, 120)
    x[torch.arange(120), torch.arange(120)] = 1.0
    got = ops.mlp_forward(packed(st), x.to(DEV), precision="f16")
    mx, mean = err(got, emu_mlp(O.to_torch(st), x))
    assert mx < 1e-4 and mean < 2e-6, (mx, mean)
    # ... and the check can tell columns apart: the emulation with two input columns swapped lies OUTSIDE the tolerance accepted above
    xs = x.clone()
    xs[:, [5, 60]] = xs[:, [60, 5]]
    assert err(got, emu_mlp(O.to_torch(st), xs))[0] > 1e-4


@torch.no_grad()
@pytest.mark.parametrize("bad", [float("inf"), float("nan"), 7e4, -7e4])
def test_f16_pack_refuses_what_fp16_cannot_hold(bad):
    st = {k: v.copy() for k, v in synth.mlp_state(3, 1.0).items()}
    st["xyz_encoding_3.0.weight"][17, 200] = bad
    with pytest.raises(ops.PackRangeError, match="fp16"):
        packed(st)
    st["xyz_encoding_3.0.weight"][17, 200] = 65504.0          # the largest finite fp16 is in range
    assert isinstance(packed(st), ops.F16Pack)
    with pytest.raises(ValueError):                            # the layouts are not interchangeable
        ops.mlp_forward(packed(st, "bf16"), embedded(4, 0).to(DEV), precision="f16")
    with pytest.raises(ValueError):
        ops.mlp_forward(packed(st), embedded(4, 0).to(DEV), precision="bf16")


@torch.no_grad()
def test_subnormal_weights_are_kept():
    """Weights below 2^-14 are fp16 subnormals.  xyz_encoding_2's weights scaled by 2^-13 (all of them subnormal or zero in fp16) and
    xyz_encoding_3's by 2^13, against the emulation with subnormal operands KEPT and with them FLUSHED to zero: the hardware keeps them."""
    st = {k: v.copy() for k, v in synth.mlp_state(7, 1.0).items()}
    st["xyz_encoding_2.0.weight"] *= 2.0 ** -13
    st["xyz_encoding_2.0.bias"] *= 2.0 ** -13
    st["xyz_encoding_3.0.weight"] *= 2.0 ** 13
    assert float(np.abs(st["xyz_encoding_2.0.weight"]).max()) < 2.0 ** -14
    x = embedded(512, 11)
    got = ops.mlp_forward(packed(st), x.to(DEV), precision="f16")
    kept = err(got, emu_mlp(O.to_torch(st), x))
    flushed = err(got, emu_mlp(O.to_torch(st), x, round_fn=f16_round_flushed))
    print("subnormal fp16 operands: vs emulation that keeps them max %.3e mean %.3e; vs emulation that flushes them max %.3e mean %.3e" % (kept + flushed))
    assert kept[0] < 1e-3 and kept[1] < 2e-6, kept
    assert flushed[1] > 2e-6, (kept, flushed)                 # ... and the bar tells the two apart: the flushing emulation misses it (measured: 1.3e-5 against 2.6e-7)


# ------------------------------------------------------------------ 4. the range guard
def _overflow_ratio(w, x):
    """Per point: max over every fp32 -> fp16 operand conversion of the MLP of value / 65,520 (>= 1: the conversion gives inf).  A negative value in
    front of a relu is not an operand (relu first); the embedded input and xyz_encoding_final's output count with their magnitude."""
    import torch.nn.functional as F
    q = f16_round
    worst = x.abs().max(1).values / F16_OVERFLOW
    lin = lambda h, name: F.linear(q(h), q(w[name + ".weight"]), w[name + ".bias"])  # noqa: E731
    xyz = x[:, :93]
    h = xyz
    for layer in range(1, 9):
        if layer == 5:
            h = torch.cat((xyz, h), 1)
        h = F.relu(lin(h, "xyz_encoding_%d.0" % layer))
        worst = torch.maximum(worst, torch.nan_to_num(h, nan=float("inf")).max(1).values / F16_OVERFLOW)
    final = lin(h, "xyz_encoding_final")
    worst = torch.maximum(worst, torch.nan_to_num(final, nan=float("inf")).abs().max(1).values / F16_OVERFLOW)
    g = F.relu(lin(torch.cat((final, x[:, 93:]), 1), "dir_encoding.0"))
    worst = torch.maximum(worst, torch.nan_to_num(g, nan=float("inf")).max(1).values / F16_OVERFLOW)
    return worst


def _guard_case():
    """A coarse model whose xyz_encoding_8 is scaled up (the weights of its two readers, static_sigma and xyz_encoding_final, by the inverse, so the
    network stays the function it was and as well conditioned: only h8 itself is large)
    such that some, not all, rays have a point whose h8 leaves fp16's range.  The scale is chosen here, on the CPU, from the emulation; rays
    with a conversion within 3 % of the overflow threshold are left out (the kernel's summation order may decide those either way)."""
    Nc = 64
    st = {k: v.copy() for k, v in synth.mlp_state(21, 2.0).items()}
    rays = torch.from_numpy(synth.rays(160, seed=5))
    zt = torch.linspace(0, 1, Nc)
    z = rays[:, 6:7] * (1 - zt) + rays[:, 7:8] * zt
    pts = (rays[:, None, 0:3] + rays[:, None, 3:6] * z[..., None]).reshape(-1, 3)
    x = torch.cat((O.posenc(pts, 15), O.posenc(rays[:, 3:6], 4).repeat_interleave(Nc, 0)), 1)
    for e in range(64, 200):                                   # scales 2^8 .. 2^25 in steps of 2^(1/8)
        f = np.float32(2.0 ** (e / 8.0))
        s = dict(st)
        s["xyz_encoding_8.0.weight"], s["xyz_encoding_8.0.bias"] = st["xyz_encoding_8.0.weight"] * f, st["xyz_encoding_8.0.bias"] * f
        s["static_sigma.0.weight"] = st["static_sigma.0.weight"] / f
        s["xyz_encoding_final.weight"] = st["xyz_encoding_final.weight"] / f      # (fp16 subnormals: kept by the kernel and by the emulation alike)
        ratio = _overflow_ratio(O.to_torch(s), x).view(-1, Nc)
        over = (ratio >= 1).any(1)
        if 0.2 <= float(over.float().mean()) <= 0.8:
            clear = ~((ratio > 0.97) & (ratio < 1.03)).any(1)
            assert int((over & clear).sum()) >= 8 and int((~over & clear).sum()) >= 8
            return s, rays[clear].contiguous(), over[clear], zt
    raise AssertionError("no scale splits the rays")


@torch.no_grad()
def test_range_guard_poisons_exactly_the_overflowing_rays_and_bf16_fc_repairs_them():
    from crnerf_amd.models.nerf import NeRF_sigma, PosEmbedding
    from crnerf_amd.models.rendering import render_rays_cross_ray
    st, rays, over, zt = _guard_case()
    Nc = 64
    out = ops.render_rays(packed(st), None, rays.to(DEV), Nc, 0, z_steps=zt.to(DEV), precision="f16")
    nan_ray = torch.isnan(out["feature_coarse"]).any(1).cpu()
    print("range guard: %d rays, %d overflow in the emulation, %d NaN from the kernel" % (len(over), int(over.sum()), int(nan_ray.sum())))
    assert torch.equal(nan_ray, over)                                            # exactly the overflowing rays ...
    assert bool(torch.isnan(out["feature_coarse"][over.to(DEV)]).all())          # ... whole feature rows (what the repair kernel looks at)
    ok = ~over
    orc = emu_render(O.to_torch(st), None, rays[ok], Nc, 0, z_steps=zt)
    for k in ("weights_coarse", "feature_coarse", "depth_coarse"):               # none finite-and-wrong
        mx, mean = err(out[k][ok.to(DEV)], orc[k])
        print("range guard, rays in range, %s: max %.3e mean %.3e" % (k, mx, mean))
        assert mx < 2e-2 and mean < 2e-4, (k, mx, mean)
    # the same through the mode: repaired by the f32x3 kernel inside the call

    class Args:
        nerf_out_dim, img_wh, pertubeCord = 64, [8, 8], False
    mk = lambda typ: NeRF_sigma(typ, Args(), in_channels_xyz=93, in_channels_dir=27).to(DEV)  # noqa: E731
    coarse, fine = mk("coarse"), mk("fine")
    coarse.load_state_dict({k: C(v) for k, v in st.items()})
    fine.load_state_dict({k: C(v) for k, v in synth.mlp_state(22, 2.0).items()})
    emb = {"xyz": PosEmbedding(14, 15), "dir": PosEmbedding(3, 4)}
    call = lambda prec: render_rays_cross_ray({"coarse": coarse, "fine": fine}, emb, rays.to(DEV), None, Nc, False, 0, 0, 128, 32768, False,  # noqa: E731
                                              test_time=True, args=Args(), precision=prec)
    fc, f32 = call("bf16_fc"), call("f32")
    for k, v in fc.items():
        assert bool(torch.isfinite(v).all()), k
    # a repaired QUAD is re-rendered whole: its rays carry the f32x3 kernel's coarse weights (fp32-accurate)
    quad_bad = over.clone()
    for q0 in range(0, len(over), 4):
        quad_bad[q0:q0 + 4] = over[q0:q0 + 4].any()
    d = (fc["weights_coarse"] - f32["weights_coarse"]).abs().max(1).values.cpu()
    print("bf16_fc: weights_coarse of the repaired rays vs f32: max %.3e; of the others: max %.3e" % (float(d[quad_bad].max()), float(d[~quad_bad].max())))
    assert float(d[quad_bad].max()) <= 1e-5
    assert torch.equal(fc["weights_coarse"][(~quad_bad).to(DEV)], out["weights_coarse"][(~quad_bad).to(DEV)])   # untouched where nothing overflowed


# ------------------------------------------------------------------ 5. the mode is what it says
def _models(seed_c=31, seed_f=32, gain=1.5):
    from crnerf_amd.models.nerf import NeRF_sigma, PosEmbedding

    class Args:
        nerf_out_dim, img_wh, pertubeCord, encode_a, encode_random = 64, [40, 24], False, True, True
        N_emb_xyz, N_emb_dir, N_a = 15, 4, 48
    mk = lambda typ: NeRF_sigma(typ, Args(), in_channels_xyz=93, in_channels_dir=27, encode_appearance=True, encode_random=True).to(DEV)  # noqa: E731
    coarse, fine = mk("coarse"), mk("fine")
    coarse.load_state_dict({k: C(v) for k, v in synth.mlp_state(seed_c, gain).items()})
    fine.load_state_dict({k: C(v) for k, v in synth.mlp_state(seed_f, gain).items()})
    return {"coarse": coarse, "fine": fine}, {"xyz": PosEmbedding(14, 15), "dir": PosEmbedding(3, 4)}, Args()


@torch.no_grad()
def test_bf16_fc_is_f16_coarse_plus_bf16_fine_bit_for_bit():
    import crnerf_amd
    from crnerf_amd.models.rendering import render_rays_cross_ray
    models, emb, args = _models()
    R, Nc, Ni = 4099, 64, 128                                  # ragged: not a multiple of the quad, of the chunk below
    rays = C(synth.rays(R, seed=9))
    zt, ut = torch.linspace(0, 1, Nc, device=DEV), torch.linspace(0, 1, Ni, device=DEV)
    call = lambda prec: render_rays_cross_ray(models, emb, rays, None, Nc, False, 0, 0, Ni, 32768, False, test_time=True, args=args, precision=prec)  # noqa: E731
    fc, f32, bf = call("bf16_fc"), call("f32"), call("bf16")
    assert list(fc.keys()) == list(f32.keys())
    direct = ops.render_rays(models["coarse"].packed_weights("f16"), None, rays, Nc, 0, z_steps=zt, precision="f16")
    assert bool(torch.isfinite(direct["feature_coarse"]).all())                  # nothing to repair here: the mode's coarse pass IS the f16 kernel's
    for k in ("weights_coarse", "feature_coarse", "depth_coarse"):
        assert torch.equal(fc[k], direct[k]), k
    assert not torch.equal(fc["weights_coarse"], f32["weights_coarse"])          # ... not the silent fall-through of an unknown precision string
    assert not torch.equal(fc["weights_coarse"], bf["weights_coarse"])
    fine = ops.render_rays_bf16_fine(models["fine"].packed_weights("bf16"), rays, direct["weights_coarse"], Nc, Ni, z_steps=zt, u=ut)
    for k in ("weights_fine", "feature_fine", "depth_fine"):
        assert torch.equal(fc[k], fine[k]), k
    assert fc["feature_fine_random"] is fc["feature_fine"]
    # the same through batched_inference in 2,048-ray chunks, by keyword and by the package-wide default
    bi = pipeline.batched_inference(models, emb, rays, None, Nc, Ni, False, 2048, False, args=args, precision="bf16_fc")
    for k in fc:
        assert torch.equal(bi[k], fc[k]), k
    crnerf_amd.set_precision("bf16_fc")
    try:
        bd = pipeline.batched_inference(models, emb, rays, None, Nc, Ni, False, 2048, False, args=args)
    finally:
        crnerf_amd.set_precision("f32")
    for k in fc:
        assert torch.equal(bd[k], fc[k]), k
    # the pack is cached and invalidated like the others
    pk = models["coarse"].packed_weights("f16")
    assert models["coarse"].packed_weights("f16") is pk
    models["coarse"].load_state_dict(models["coarse"].state_dict())
    assert models["coarse"].packed_weights("f16") is not pk
    # outside the mode's applicability (no fine pass): the path plain bf16 takes
    c_only = render_rays_cross_ray(models, emb, rays, None, Nc, False, 0, 0, 0, 32768, False, test_time=True, args=args, precision="bf16_fc")
    b_only = render_rays_cross_ray(models, emb, rays, None, Nc, False, 0, 0, 0, 32768, False, test_time=True, args=args, precision="bf16")
    assert torch.equal(c_only["feature_coarse"], b_only["feature_coarse"])


@torch.no_grad()
def test_bf16_fc_falls_back_to_bf16_hc_when_the_weights_do_not_fit_fp16():
    import warnings
    from crnerf_amd.models import rendering
    from crnerf_amd.models.rendering import render_rays_cross_ray
    models, emb, args = _models()
    with torch.no_grad():
        models["coarse"].xyz_encoding_1[0].weight[3, 90] = 7e4      # an identity column of the embedding: finite everywhere, but not an fp16 number
    models["coarse"].invalidate_packed()
    rays = C(synth.rays(64, seed=1))
    call = lambda prec: render_rays_cross_ray(models, emb, rays, None, 64, False, 0, 0, 128, 32768, False, test_time=True, args=args, precision=prec)  # noqa: E731
    rendering._warned_f16_refused[0] = False
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        fc = call("bf16_fc")
        call("bf16_fc")
    assert sum("does not fit fp16" in str(w.message) for w in rec) == 1          # said once
    hc = call("bf16_hc")
    for k in fc:
        assert torch.equal(fc[k], hc[k]), k

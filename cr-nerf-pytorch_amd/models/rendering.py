"""render_rays_cross_ray with the reference's signature (models/rendering.py:50-63) on the fused HIP
renderer.  Callers: train_mask_grid_sample.py:185-197, eval.py:39-52,
appearance_modification_video.py:82-95 -- all pass the first 11 arguments positionally."""
from typing import NamedTuple

import torch

from .. import ops
from ..precision import COMPOSITE, resolve
from .nerf import NeRF_sigma, PosEmbedding

__all__ = ['render_rays_cross_ray', 'render_route', 'RenderRoute']

_FUSED_MAX = 256


def _coarse_depths(rays, N_samples, use_disp, perturb):
    """Stratified coarse depths for perturb > 0 (models/rendering.py:161-176), drawn with torch's RNG."""
    near, far = rays[:, 6:7], rays[:, 7:8]
    s = torch.linspace(0, 1, N_samples, device=rays.device)
    z = near * (1 - s) + far * s if not use_disp else 1 / (1 / near * (1 - s) + 1 / far * s)
    z = z.expand(rays.shape[0], N_samples)
    mid = 0.5 * (z[:, :-1] + z[:, 1:])
    upper = torch.cat([mid, z[:, -1:]], -1)
    lower = torch.cat([z[:, :1], mid], -1)
    return (lower + (upper - lower) * (perturb * torch.rand_like(z))).contiguous()


_tables = {}


def _linspace_tables(n_samples, n_importance, device):
    """The reference's two tables, built the reference's way on the same device (rendering.py:160, :27)."""
    key = (n_samples, n_importance, str(device))
    if key not in _tables:
        _tables[key] = (torch.linspace(0, 1, n_samples, device=device),
                        torch.linspace(0, 1, n_importance, device=device) if n_importance > 0 else None)
    return _tables[key]


def _render_unfused(coarse, fine, rays, Nc, Ni, use_disp, view_dir, z_coarse, u, noise_c, noise_f, noise_std, jitter, chunk, train=False,
                    precision="f32", plan=None):
    """train: `plan` is the caller's autograd.TrainPlan (None: resolved here, once for every MLP call of this render)."""
    if train:   # autograd.Functions over the HIP forward/backward twins (autograd.py)
        from ..autograd import CompositeFn, mlp_forward_with_grad, training_plan
        plan = plan or training_plan()
    R = rays.shape[0]
    o, d = rays[:, None, 0:3], rays[:, None, 3:6]
    z_steps, u_steps = _linspace_tables(Nc, Ni, rays.device)
    if z_coarse is None:
        near, far = rays[:, 6:7], rays[:, 7:8]
        z_coarse = (near * (1 - z_steps) + far * z_steps) if not use_disp else 1 / (1 / near * (1 - z_steps) + 1 / far * z_steps)
        z_coarse = z_coarse.expand(R, Nc).contiguous()
    demb = ops.posenc((view_dir if view_dir is not None else rays[:, 3:6]).contiguous(), 4)

    def run(model, z, noise):
        N = z.shape[1]
        # point chunks (rendering.py:110-114) only bound the reference's activation memory; the result is chunk-invariant
        # (SURVEY G7), and every MLP call here costs a weight re-pack (+ a wgrad reduction in training), so never go below 2^20 points
        step = max(int(chunk), 1 << 20)
        with torch.no_grad():                                                # embeddings are inputs, not trained
            if jitter:
                pts = (o + d * z[..., None]).reshape(-1, 3)
                pts = pts + 0.00001 * torch.rand_like(pts)                   # rendering.py:102-104
                dirs = demb[:, None, :].expand(R, N, demb.shape[-1]).reshape(R * N, -1)
                xs = [torch.cat([ops.posenc(pts[i:i + step].contiguous(), 15), dirs[i:i + step]], 1) for i in range(0, R * N, step)]
            else:   # the same rows in one pass per ray block (crnerf_embed_points_f32): points, embedding, repeat and cat fused
                rstep = max(step // N, 1)
                zc = z.contiguous()
                xs = [ops.embed_points(rays[i:i + rstep], zc[i:i + rstep], demb[i:i + rstep]) for i in range(0, R, rstep)]
        if train:
            raw = torch.cat([mlp_forward_with_grad(model, x, plan) for x in xs], 0)
            return CompositeFn.apply(raw.view(R, N, 65), z.contiguous(), noise, noise_std)
        raw = torch.cat([ops.mlp_forward(model.packed_weights(precision), x, precision=precision) for x in xs], 0)   # point chunks, rendering.py:110-114
        return ops.composite(raw.view(R, N, 65), z.contiguous(), noise, noise_std)

    out = {}
    out["weights_coarse"], out["feature_coarse"], out["depth_coarse"] = run(coarse, z_coarse, noise_c)
    if Ni > 0:
        z_fine = ops.sample_pdf_merge(z_coarse.contiguous(), out["weights_coarse"].detach(), Ni,   # .detach(): rendering.py:184
                                      u=u if u is not None else u_steps)
        out["weights_fine"], out["feature_fine"], out["depth_fine"] = run(fine, z_fine, noise_f)
    return out


_warned_f16_refused = [False]


def _render_bf16_composite(coarse, fine, rays, Nc, Ni, use_disp, view_dir, noise_c, noise_f, noise_std, route, want_z_fine=False):
    """precision="bf16_hc" (inference, perturb = 0): the COARSE pass in fp32 accuracy on the fp16 matrix cores (precision "auto": f32h2 with the
    f32x3 safety net; 25 % of the points), the FINE pass on the bf16 matrix cores.  Why: bf16's end-to-end pixel error on a trained checkpoint is
    sampling sensitivity -- bf16 coarse weights move the fine depths (weights_fine rel-L2 2.8e-2, tests/test_gpu_trained_ckpt.py) -- so with
    fp32-accurate coarse weights the fine depths are the fp32 reference's and what is left is the fine network's own bf16 rounding.
    Two fused launches (+ the repair kernel that leaves at once): the coarse-only render on the h2 core, then crnerf_render_rays_bf16_fine --
    sample_pdf, merge, embedding, fine MLP and compositing in one kernel on the coarse weights (round 6; rounds 4-5 ran five un-fused calls with
    the [P,120] embeddings and [P,65] raw rows through HBM: 297 ms per 800 x 800 frame).
    route.f16_coarse: precision="bf16_fc", the same with the coarse pass on ONE-PIECE FP16 operands -- one MFMA per product like bf16 instead of the h2
    core's three, 11 significand bits instead of bf16's 8: the coarse weights, and with them the fine depths, land ~7x closer to fp32's than bf16's
    do (tests/test_gpu_f16_trained.py) at bf16's cost.  Three launches: the coarse-only crnerf_render_rays_f16, crnerf_render_rays_f32x3_repair over
    its outputs (re-renders the ray quads the fp16 range guard poisoned; leaves at once otherwise -- so the mode returns no NaN that "f32" would
    not), crnerf_render_rays_bf16_fine on those coarse weights.  A coarse model whose weights do not fit fp16 (the pack refuses them) takes
    bf16_hc's coarse pass instead; said once in a warning.
    route.lean_launch: the caller reads the fine image alone.  The coarse launch becomes ops.render_coarse_weights (crnerf_render_coarse_weights_f32h2 / _f16 + the
    x3 repair: every tile stops behind the sigma head, weights_coarse is all it writes, bit-identical to the ordinary launch's) and the fine launch
    crnerf_render_rays_lean_bf16_fine (no weights_fine); the dict holds feature_fine, depth_fine and (want_z_fine) z_fine."""
    # how the coarse pass is obtained: its precision, its pack and (f16) the x3 pack of the repair behind it
    precision, pk, repair = "auto", None, None
    if route.f16_coarse:
        try:
            precision, pk = "f16", coarse.packed_weights("f16")
        except ops.PackRangeError:
            if not _warned_f16_refused[0]:
                _warned_f16_refused[0] = True
                import warnings
                warnings.warn("crnerf_amd: precision='bf16_fc': a weight of the coarse model does not fit fp16 (|w| <= 65,504, finite); "
                              "its coarse pass runs as in 'bf16_hc'")
    z_steps, u_steps = _linspace_tables(Nc, Ni, rays.device)
    if pk is None:
        pk = coarse.packed_weights("auto")
    else:
        repair = coarse.packed_weights("f32x3")
    kw = dict(use_disp=use_disp, z_steps=z_steps, noise_coarse=noise_c, noise_std=float(noise_std), precision=precision)
    if route.lean_launch:
        out = {}
        wc = ops.render_coarse_weights(pk, rays, Nc, repair_x3=repair, **kw)["weights_coarse"]
    else:     # (view_dir: the full launch also composites feature_coarse)
        out = ops.render_rays(pk, None, rays, Nc, 0, view_dir=view_dir, repair_x3=None if repair is None else (repair, None), **kw)
        wc = out["weights_coarse"]
    out.update(ops.render_rays_bf16_fine(fine.packed_weights("bf16"), rays, wc, Nc, Ni, use_disp=use_disp, view_dir=view_dir, z_steps=z_steps, u=u_steps,
                                         noise_fine=noise_f, noise_std=float(noise_std), want_z_fine=want_z_fine, lean=route.lean_launch))
    return out


class RenderRoute(NamedTuple):
    """Which launch a render_rays_cross_ray call gets -- everything its dispatch reads (render_route)."""
    path: str            # "train_fused" | "composite" | "unfused" | "lean_x" | "fused": a row of render_rays_cross_ray's table
    precision: str       # the name the packs and launchers are handed
    lean: bool           # the caller reads the fine image alone: the result holds nothing else
    lean_launch: bool    # ... and the launch itself is lean (False under lean: rendered in full, the rest dropped)
    f16_coarse: bool     # "composite": the coarse pass on one-piece fp16 operands ("bf16_fc")
    kernel_draws: bool   # jitter / sample_pdf uniforms / density noise are drawn in the kernel (csrc/philox.h), not handed over as tensors


def _fits_fused(n_samples, n_importance, short=False):
    """The fused kernels' sample counts (their LDS scratch; sample_pdf needs three coarse samples).  short: N_samples < 3 is accepted as well."""
    return (short or n_samples >= 3) and n_samples <= _FUSED_MAX and n_importance <= _FUSED_MAX


def render_route(precision, train, plan, jitter, perturb, noise_std, n_samples, n_importance, lean, in_kernel_rng):
    """The RenderRoute of a call, from plain values alone: precision -- its canonical name (crnerf_amd.precision.resolve); train -- grad mode with
    trainable models; plan -- autograd.training_plan()'s answer (read only when train); jitter -- args.pertubeCord; in_kernel_rng -- what
    ops.in_kernel_rng() answers.  Every sample-count rule that is not _fits_fused() as it stands carries its reason."""
    lean = lean and n_importance > 0        # without a fine pass the flag means nothing
    if train:                               # grad mode does not read the precision setting (crnerf_amd.set_precision): the plan decides
        # short: the training twin runs sample_pdf only when there is a fine pass
        fusable = not jitter and _fits_fused(n_samples, n_importance, short=n_importance == 0)
        fused_f32 = fusable and plan.family == "f32"
        if fused_f32 or (fusable and (plan.recompute or plan.bf16_fused)):
            # only the fp32 family's training kernel draws for itself
            return RenderRoute("train_fused", "f32", False, False, False, fused_f32 and (perturb > 0 or noise_std != 0) and in_kernel_rng)
        return RenderRoute("unfused", "f32", False, False, False, False)
    if precision in COMPOSITE and n_importance > 0 and perturb == 0 and not jitter:
        # "bf16_hc" does not bound N_importance although its fine launch does -- a defect, kept as it is: N_importance > 256 is refused
        # by ops.render_rays_bf16_fine where "bf16_fc" one line on renders un-fused
        if _fits_fused(n_samples, 0 if precision == "bf16_hc" else n_importance):
            return RenderRoute("composite", "bf16", lean, lean, precision == "bf16_fc", False)
    if precision in COMPOSITE:              # outside their applicability the composite modes take the path plain "bf16" takes
        precision = "bf16"
    if jitter or not _fits_fused(n_samples, n_importance, short=True):      # short: the un-fused path is for counts beyond the scratch, not below it
        return RenderRoute("unfused", precision, lean, False, False, False)
    lean_launch = lean and _fits_fused(n_samples, n_importance)             # the full entries render N_samples < 3, the lean entries do not
    return RenderRoute("lean_x" if lean_launch and precision in ("f32x3", "f32h2", "auto") else "fused", precision, lean, lean_launch, False, False)


def _check_embedding(emb, n_freqs, what):
    if not isinstance(emb, PosEmbedding) or emb.N_freqs != n_freqs:
        raise NotImplementedError("crnerf_amd: embeddings['%s'] must be crnerf_amd PosEmbedding(%d, %d); the fused kernel computes "
                                  "the embedding in registers and cannot call an arbitrary Python callable" % (what, n_freqs - 1, n_freqs))


def _results(out, coarse, fine, route, output_random):
    """The reference's result names (models/rendering.py:140-141,192) for a launch dict; route.lean: the fine image alone."""
    typ = coarse.typ
    results = {} if route.lean else {'weights_%s' % typ: out['weights_coarse'], 'feature_%s' % typ: out['feature_coarse'],
                                     'depth_%s' % typ: out['depth_coarse']}
    if fine is not None:
        if not route.lean:
            results['weights_%s' % fine.typ] = out['weights_fine']
        results['feature_%s' % fine.typ] = out['feature_fine']
        if output_random and fine.encode_random:
            results['feature_fine_random'] = out['feature_fine']         # the SAME tensor object, as in the reference
        results['depth_%s' % fine.typ] = out['depth_fine']
    return results


def render_rays_cross_ray(models, embeddings, rays, ts, N_samples=64, use_disp=False, perturb=0, noise_std=1,
                          N_importance=0, chunk=1024 * 32, white_back=False, test_time=False, **kwargs):
    """Same contract as the reference: returns weights_/feature_/depth_ for 'coarse' and, when N_importance > 0, 'fine' (+ 'feature_fine_random', the
    SAME tensor object as 'feature_fine', models/rendering.py:140-141,192).  ts / white_back / test_time / chunk are accepted and, as in the
    reference's arithmetic, do not influence the result (the MLP is point-wise, so chunking is invisible).
    Keywords beyond the reference's: precision (a name of crnerf_amd.precision, default crnerf_amd.get_precision()): the matrix-core arithmetic of
    NeRF_sigma at inference; view_dir; output_random; rng_ray_offset (below); lean=True: the caller reads the fine image alone -- the result holds
    exactly feature_<fine.typ>, depth_<fine.typ> and (under its usual condition) feature_fine_random, with the values of the ordinary call; inference
    only (ValueError in grad mode with trainable models), meaningless with N_importance == 0, not tied to test_time, which every inference caller sets.
    Grad mode with trainable models reads autograd.training_plan() instead of the precision.

    The launch a call gets -- render_route() decides, first match wins; "counts fit": 3 <= N_samples <= 256 and N_importance <= 256:

    | route       | condition                                             | launch                                        | entries documented in           | a lean call                |
    |-------------|-------------------------------------------------------|-----------------------------------------------|---------------------------------|----------------------------|
    | train_fused | grad mode, no pertubeCord, counts fit (N_samples < 3  | autograd.fused_render_with_grad: one autograd | autograd.FusedRenderFn,         | is refused: ValueError     |
    |             | too when N_importance == 0); plan: f32 family,        | node per ray chunk                            | include/crnerf.h                |                            |
    |             | recompute or bf16 fused                               |                                               |                                 |                            |
    | unfused     | grad mode otherwise                                   | _render_unfused on the autograd twins         | autograd.py                     | is refused: ValueError     |
    | composite   | "bf16_hc" / "bf16_fc", N_importance > 0, perturb == 0,| _render_bf16_composite: ops.render_rays       | include/crnerf.h,               | ops.render_coarse_weights, |
    |             | no pertubeCord, counts fit ("bf16_hc": N_importance   | (coarse only), ops.render_rays_bf16_fine      | include/crnerf_lean_composite.h | the fine launch lean       |
    |             | not bounded)                               |                                               |                                 |                            |
    | unfused     | pertubeCord, N_samples > 256 or N_importance > 256    | _render_unfused on ops.mlp_forward            | include/crnerf.h                | renders in full, drops     |
    | lean_x      | lean, "f32x3" / "f32h2" / "auto", N_samples >= 3      | ops.render_rays_lean_x                        | include/crnerf_lean_x.h         | is what this row is for    |
    | fused       | everything else ("bf16_hc" / "bf16_fc" as "bf16")     | ops.render_rays                               | include/crnerf.h,               | lean=True; N_samples < 3:  |
    |             |                                                       |                                               | include/crnerf_lean.h           | renders in full, drops     |

    What an entry does with NaN rows and fp16's range guard is said where the entry is: the docstrings of ops.render_rays, ops.render_rays_lean_x,
    ops.render_coarse_weights, ops.render_rays_bf16_fine and _render_bf16_composite, and the headers above.
    Random inputs (perturb > 0: stratified coarse depths and sample_pdf's uniforms; noise_std != 0: density noise) are torch draws handed on as tensors,
    except where the route says kernel_draws (train_fused on the f32 plan with ops.in_kernel_rng()): then the only draw is the Philox seed, from torch's
    CPU generator, so torch.manual_seed() governs the run either way.  rng_ray_offset: the index of rays[0] in the caller's whole batch -- the kernel's
    draws are keyed on (seed, GLOBAL ray, sample), so a batch rendered in ray chunks or sharded over ranks (pipeline.TrainingSystem) draws what one
    call over all of it would."""
    args = kwargs['args']
    jitter = bool(getattr(args, 'pertubeCord', False))
    if getattr(args, 'nerf_out_dim', 64) != 64:
        raise NotImplementedError("crnerf_amd: nerf_out_dim must be 64")
    _check_embedding(embeddings['xyz'], 15, 'xyz')
    _check_embedding(embeddings['dir'], 4, 'dir')
    coarse = models['coarse']
    fine = models.get('fine') if N_importance > 0 else None
    for m in (coarse, fine):
        if m is not None and not isinstance(m, NeRF_sigma):
            raise NotImplementedError("crnerf_amd: models must be crnerf_amd NeRF_sigma instances")
    train = torch.is_grad_enabled() and any(ops.any_requires_grad(m) for m in (coarse, fine) if m is not None)
    lean = bool(kwargs.get('lean', False))
    if lean and train:
        raise ValueError("crnerf_amd: lean=True is an inference render; call it under torch.no_grad() (or with frozen models)")
    precision = kwargs.get('precision', None)
    if precision is None:
        from .. import get_precision
        precision = get_precision()
    from ..autograd import fused_render_with_grad, training_plan
    plan = training_plan() if train else None      # the training settings, asked once: this call's nodes run as it says, forward and backward
    route = render_route("f32" if train else resolve(precision, composite=True), train, plan, jitter, perturb, noise_std, N_samples, N_importance, lean,
                         train and ops.in_kernel_rng())      # (asked in grad mode only: no inference launch draws for itself)

    rays = rays.to(torch.float32).contiguous()
    R = rays.shape[0]
    view_dir = kwargs.get('view_dir', None)
    noise_std = float(noise_std)
    rng = z_coarse = u = noise_c = noise_f = None
    if route.kernel_draws:
        rng = {"seed": int(torch.randint(0, 2 ** 62, (1,), device="cpu")), "perturb": float(perturb), "jitter": perturb > 0, "u": perturb > 0,
               "noise": noise_std != 0, "ray_offset": int(kwargs.get("rng_ray_offset", 0))}
    else:
        if perturb > 0:
            z_coarse = _coarse_depths(rays, N_samples, use_disp, perturb)
            if N_importance > 0:
                u = torch.rand(R, N_importance, device=rays.device)
        if noise_std != 0:
            noise_c = torch.randn(R, N_samples, device=rays.device)
            if N_importance > 0:
                noise_f = torch.randn(R, N_samples + N_importance, device=rays.device)

    if route.path == "train_fused":
        out = fused_render_with_grad(coarse, fine, rays, N_samples, N_importance, use_disp, view_dir, z_coarse, u, noise_c, noise_f, noise_std, rng=rng,
                                     plan=plan)
    elif route.path == "composite":
        out = _render_bf16_composite(coarse, fine, rays, N_samples, N_importance, use_disp, view_dir, noise_c, noise_f, noise_std, route)
    elif route.path == "unfused":
        out = _render_unfused(coarse, fine, rays, N_samples, N_importance, use_disp, view_dir, z_coarse, u, noise_c, noise_f, noise_std, jitter,
                              int(chunk), train, route.precision, plan)
    else:
        z_steps, u_steps = _linspace_tables(N_samples, N_importance, rays.device)
        render, flag = (ops.render_rays_lean_x, {}) if route.path == "lean_x" else (ops.render_rays, {"lean": route.lean_launch})
        out = render(coarse.packed_weights(route.precision), fine.packed_weights(route.precision) if fine is not None else None, rays, N_samples,
                     N_importance, precision=route.precision, use_disp=use_disp, view_dir=view_dir, z_coarse=z_coarse, z_steps=z_steps,
                     u=u if u is not None else u_steps, noise_coarse=noise_c, noise_fine=noise_f, noise_std=noise_std, **flag)
    return _results(out, coarse, fine, route, kwargs.get('output_random', True))

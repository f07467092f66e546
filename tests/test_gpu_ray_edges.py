"""sample_pdf, the z merge and compositing at their edges, against float64 (tests/_ray_cases.py holds the inputs, the references and where
every bound comes from; tests/test_ray_edges_host.py shows the fp32 CPU oracle meets the same bounds on the same inputs).

Two hand-written copies of the sampler and the merge exist -- sample_pdf_wave / merge_sort_wave (csrc/ray_ops.h, one wave per ray: the
stand-alone crnerf_sample_pdf_merge_f32 and the x3 / h2 renderers) and sample_pdf_pair / merge_sort_pair (csrc/pair_ops.h, two waves per ray: the
fp32, lean, bf16 and f16 renderers).  The stand-alone kernel is pinned to float64 here, at every size where the cdf scan or the merge takes
another path; the fused renderers are then pinned to the stand-alone kernel bit for bit."""
import numpy as np
import pytest
import torch

import _ray_cases as RC
import crnerf_amd.synth as synth
from crnerf_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def D(t):
    return None if t is None else t.to(DEV)


def sorted_cat(zc, smp):
    return torch.sort(torch.cat((zc, smp.cpu()), 1), 1)[0]


def run(zc, w, ni, u):
    zs, smp = ops.sample_pdf_merge(D(zc), D(w), ni, u=D(u), return_samples=True)
    return zs.cpu(), smp.cpu()


# ------------------------------------------------------------------ crnerf_sample_pdf_merge_f32 against float64
@torch.no_grad()
@pytest.mark.parametrize("nc,ni", RC.SHAPES)
@pytest.mark.parametrize("family", RC.FAMILIES)
def test_sample_pdf_merge_vs_float64(family, nc, ni):
    """(3, 5): one pdf bin; (65, 65) / (66, 128): 63 / 64 bins, the last sizes of a one-chunk cdf scan; (67, 129): 65 bins, the first carry from
    chunk to chunk; (256, 256): four chunks."""
    zc, w, u = RC.sample_case(family, nc, ni)
    zs, smp = run(zc, w, ni, u)
    st = RC.check_samples(smp, zc, w, u, RC.K_KERNEL, min_share=RC.MIN_PINNED_SHARE, what="%s (%d, %d)" % (family, nc, ni))
    print("sample_pdf_merge %-8s (%3d, %3d): pinned share %.3f, K needed %.3f of %.2f, largest pinned error %.3g" % (family, nc, ni, st["share"],
                                                                                                                st["k_needed"], RC.K_KERNEL, st["max_err"]))
    assert torch.equal(zs, sorted_cat(zc, smp))      # the merge is exact: a permutation of its inputs, ascending


def exact_knot_weights(n_rays, nc, g):
    """Weights whose cdf is known exactly whatever the order of the sums: every w + eps is a multiple of 2^-16, they add up to 16, so each pdf
    value and each partial sum is exact in fp32.  About half the bins hold 2^-16 (pdf 2^-20 < eps: the `denom = 1` branch), the rest small
    multiples of a power of two, one of them the remainder.  Returns (weights [R,nc] fp32, cdf [R,nc-1] fp32)."""
    m = nc - 2
    eps = torch.tensor(1e-5, dtype=torch.float32)
    unit = 2.0 ** np.floor(np.log2(4.0 / m))
    c = torch.full((n_rays, m), 2.0 ** -16, dtype=torch.float64)
    big = torch.rand(n_rays, m, generator=g) < 0.5
    big[torch.arange(n_rays), torch.randint(0, m, (n_rays,), generator=g)] = True
    c = torch.where(big, unit * torch.randint(1, 4, (n_rays, m), generator=g).double(), c)
    filler = big.double().argmax(1)
    c[torch.arange(n_rays), filler] = 0.0
    c[torch.arange(n_rays), filler] = 16.0 - c.sum(1)
    assert bool((c > 0).all()) and bool((c.sum(1) == 16.0).all())
    w = (c - eps.double()).float()
    assert torch.equal((w + eps).double(), c) and bool((w > 0).all())          # fp32: w + eps lands on c exactly
    cdf = torch.cat((torch.zeros(n_rays, 1, dtype=torch.float64), torch.cumsum(c / 16.0, 1)), 1)
    assert torch.equal(cdf.float().double(), cdf) and bool((cdf[:, -1] == 1.0).all())
    ends = torch.rand(n_rays, 2, generator=g)
    return torch.cat((ends[:, :1], w, ends[:, 1:]), 1).contiguous(), cdf.float()


@torch.no_grad()
@pytest.mark.parametrize("nc", [3, 4, 66, 67, 130, 256])
def test_u_on_a_cdf_knot_gives_that_knots_midpoint_exactly(nc):
    """searchsorted(right=True): u == cdf[j] belongs to the bin that STARTS at knot j, so the sample is midpoint j exactly (u - cdf[j] == 0), and
    u == cdf[-1] == 1 is the last midpoint.  With `<` in place of `<=` the sample would come from the bin that ends there -- for a bin on the
    `denom = 1` branch that is a whole bin width away.  Every knot of every ray is asked for, in shuffled order."""
    g = RC.generator(nc, 41)
    zc = RC.depths(RC.R, nc, g)
    w, cdf = exact_knot_weights(RC.R, nc, g)
    u = RC.shuffle_rows(cdf, g)
    zs, smp = run(zc, w, nc - 1, u)
    want = RC.midpoints(zc).gather(1, torch.searchsorted(cdf.contiguous(), u, right=True).sub(1).clamp_max(nc - 2))
    assert torch.equal(smp, want)
    assert torch.equal(zs, sorted_cat(zc, smp))


@torch.no_grad()
@pytest.mark.parametrize("family", RC.FAMILIES)
@pytest.mark.parametrize("nc,ni", [(3, 5), (67, 129), (256, 256)])
def test_u_zero_and_u_past_the_end_are_the_end_midpoints_exactly(family, nc, ni):
    zc, w, _ = RC.sample_case(family, nc, ni)
    mid = RC.midpoints(zc)
    zs, smp = run(zc, w, ni, torch.zeros(RC.R, ni))
    assert torch.equal(smp, mid[:, :1].expand(RC.R, ni))
    assert torch.equal(zs, sorted_cat(zc, smp))
    # u >= cdf[-1]: fp32's cdf ends within a few ulp of 1
    zs, smp = run(zc, w, ni, torch.full((RC.R, ni), 1.0 + 1e-3))
    assert torch.equal(smp, mid[:, -1:].expand(RC.R, ni))
    assert torch.equal(zs, sorted_cat(zc, smp))


def check_u_one(smp_at_one, zc, w):
    """u == 1.0 may land on either side of the fp32 cdf's last knot: exactly the last midpoint (u >= cdf[-1]), or the value interpolated inside
    the last bin -- held to the pinned bound where that bin is pinned (gap >= 1e-3 or <= 5e-6), to the bin's interval otherwise."""
    n_rays, m = zc.shape[0], zc.shape[1] - 2
    mid = RC.midpoints(zc).double()
    wi = w[:, 1:-1].double() + 1e-5
    cdf = torch.cat((torch.zeros(n_rays, 1, dtype=torch.float64), torch.cumsum(wi / wi.sum(1, keepdim=True), 1)), 1)
    gap, width = (cdf[:, m] - cdf[:, m - 1])[:, None], (mid[:, m] - mid[:, m - 1])[:, None]
    interp = mid[:, m - 1, None] + (1.0 - cdf[:, m - 1, None]) / torch.where(gap < 1e-5, torch.ones_like(gap), gap) * width
    z = smp_at_one.double()
    exact = smp_at_one == RC.midpoints(zc)[:, -1:]
    err = (z - interp).abs()
    pinned = (gap >= RC.GAP_WELL) | (gap <= RC.GAP_FLAT)
    ok = exact | (pinned & (err <= RC.pinned_bound(interp, gap, width, RC.K_KERNEL))) | (~pinned & (err <= width + RC.LOOSE))
    assert bool(ok.all()), "u = 1: %d samples are neither the last midpoint nor the last bin's interpolated value" % int((~ok).sum())


@torch.no_grad()
@pytest.mark.parametrize("family", RC.FAMILIES)
@pytest.mark.parametrize("nc,ni", [(3, 5), (67, 129), (256, 256)])
def test_u_exactly_one(family, nc, ni):
    zc, w, _ = RC.sample_case(family, nc, ni)
    zs, smp = run(zc, w, ni, torch.ones(RC.R, ni))
    check_u_one(smp, zc, w)
    assert torch.equal(zs, sorted_cat(zc, smp))


@torch.no_grad()
@pytest.mark.parametrize("nc", [7, 67, 130])
def test_rows_of_zeros_and_ones_many_equal_samples_on_the_rank_counting_path(nc):
    """Ni = 7, u a shuffled row of 0s and 1s: unsorted, so the merge counts ranks (count_before), with tails of 3 in both arrays and up to
    seven equal fine samples."""
    ni = 7
    g = RC.generator(nc, 7, 7)
    u = (torch.rand(RC.R, ni, generator=g) < 0.5).float()
    u[:, 0], u[:, 1], u[:, 2] = 1.0, 0.0, 1.0          # unsorted in every row
    # on a cdf known exactly (it ends at 1.0): nothing but the two end midpoints
    zc = RC.depths(RC.R, nc, g)
    w, _ = exact_knot_weights(RC.R, nc, g)
    mid = RC.midpoints(zc)
    zs, smp = run(zc, w, ni, u)
    assert torch.equal(smp, torch.where(u == 0, mid[:, :1], mid[:, -1:]))
    assert torch.equal(zs, sorted_cat(zc, smp))
    for family in ("smooth", "blocks", "surface"):
        zc, w, _ = RC.sample_case(family, nc, ni)
        mid = RC.midpoints(zc)
        zs, smp = run(zc, w, ni, u)
        assert torch.equal(smp[u == 0], mid[:, :1].expand(RC.R, ni)[u == 0])
        ones = torch.where(u == 1, smp, mid[:, -1:])     # the u == 0 entries pass as "exactly the last midpoint"
        check_u_one(ones, zc, w)
        assert torch.equal(zs, sorted_cat(zc, smp))


@torch.no_grad()
@pytest.mark.parametrize("shuffled_u", [False, True])
@pytest.mark.parametrize("nc,ni", [(7, 5), (66, 63), (130, 129)])
def test_ties_between_coarse_and_fine_depths(nc, ni, shuffled_u):
    """z_coarse in runs of 2-5 equal depths: ties inside the coarse array, and -- a sample in a zero-width bin IS that coarse depth -- between
    the two arrays.  Two entries given one rank would leave a slot of zs holding the previous ray's value.  linspace u: both arrays ascending,
    the binary-search merge; shuffled u: rank counting.  Lengths off the multiple of 4."""
    g = RC.generator(nc, ni, 13)
    zc = RC.tied_depths(RC.R, nc, g)
    w = RC.weights("smooth", RC.R, nc, g)
    u = torch.linspace(0, 1, ni).expand(RC.R, ni).contiguous()
    if shuffled_u:
        u = RC.shuffle_rows(u, g)
    zs, smp = run(zc, w, ni, u)
    assert torch.equal(zs, sorted_cat(zc, smp))
    RC.check_samples(smp, zc, w, u, RC.K_KERNEL, what="ties (%d, %d)" % (nc, ni))
    tied = (smp[:, :, None] == zc[:, None, :]).any(2)
    if nc >= 66:
        assert float(tied.float().mean()) > 0.3, "the case lost its coarse-fine ties"
        assert bool((tied.sum(1) >= 2).all())


@torch.no_grad()
@pytest.mark.parametrize("tied", [False, True])
@pytest.mark.parametrize("nc,ni", [(7, 5), (66, 63), (130, 129)])
def test_unsorted_coarse_depths_take_the_rank_counting_path(nc, ni, tied):
    g = RC.generator(nc, ni, 17, tied)
    zc = RC.shuffle_rows(RC.tied_depths(RC.R, nc, g) if tied else RC.depths(RC.R, nc, g), g)
    w = RC.weights("smooth", RC.R, nc, g)
    u = torch.rand(RC.R, ni, generator=g)
    zs, smp = run(zc, w, ni, u)
    assert bool(torch.isfinite(smp).all())
    assert torch.equal(zs, sorted_cat(zc, smp))


@torch.no_grad()
@pytest.mark.parametrize("family", ["smooth", "blocks"])
@pytest.mark.parametrize("ni", [1, 2, 63, 129])
def test_in_kernel_linspace_vs_the_table(family, ni):
    """u=None draws linspace(0, 1, Ni) in the kernel; it may differ from torch.linspace's table by 1 ulp of u = 2^-24 at most, half a unit of K."""
    nc = 67
    zc, w, _ = RC.sample_case(family, nc, ni)
    table = torch.linspace(0, 1, ni)
    _, tab = run(zc, w, ni, table)
    zs, own = ops.sample_pdf_merge(D(zc), D(w), ni, return_samples=True)
    own, ref_u = own.cpu(), table
    if ni > 1:      # the last sample is u = 1, on the cdf's last knot: check_u_one's rule for it, the pinned bound for the rest
        check_u_one(own[:, -1:], zc, w)
        check_u_one(tab[:, -1:], zc, w)
        own, tab, ref_u = own[:, :-1], tab[:, :-1], table[:-1]
    RC.check_samples(tab, zc, w, ref_u, RC.K_KERNEL, what="table, Ni = %d" % ni)
    RC.check_samples(own, zc, w, ref_u, RC.K_KERNEL + 1.0, what="in-kernel linspace, Ni = %d" % ni)
    if ni == 1:
        assert torch.equal(own, RC.midpoints(zc)[:, :1]) and torch.equal(tab, RC.midpoints(zc)[:, :1])
    assert bool((zs[:, 1:] >= zs[:, :-1]).all())


@torch.no_grad()
def test_grid_stride_loop_rows_equal_the_rows_computed_alone():
    """More rays than workgroups (8192): a workgroup walks rays r, r + 8192 with one LDS scratch.  Every row must be what a call on that row's
    neighbourhood alone gives, bit for bit -- stale scratch from the previous ray would show here.  Ties included (a zero-width bin per ray)."""
    nc, ni, n_rays = 5, 3, 8192 + 37
    g = RC.generator(nc, ni, n_rays)
    zc = RC.depths(n_rays, nc, g)
    zc[:, 2] = zc[:, 1]
    zc[1::2, 3] = zc[1::2, 2]                      # every other ray: bin 0 AND bin 1 of zero width
    w = torch.rand(n_rays, nc, generator=g) * (torch.rand(n_rays, nc, generator=g) < 0.7)
    u = torch.rand(n_rays, ni, generator=g)
    u[::3, 0] = 0.0
    zs, smp = run(zc, w, ni, u)
    assert torch.equal(zs, sorted_cat(zc, smp))
    for lo, hi in ((8192, n_rays), (0, 37), (4000, 4100), (8191, 8193)):
        zs1, smp1 = run(zc[lo:hi].contiguous(), w[lo:hi].contiguous(), ni, u[lo:hi].contiguous())
        assert torch.equal(zs1, zs[lo:hi]) and torch.equal(smp1, smp[lo:hi]), (lo, hi)
    RC.check_samples(smp[:64], zc[:64], w[:64], u[:64], RC.K_KERNEL, what="grid stride")


# ------------------------------------------------------------------ the fused renderers use what is pinned above
_PACKS = {}


def packs(precision):
    """An h2-packable net (tests/test_gpu_h2.py renders it on the h2 core), packed once per precision."""
    if precision not in _PACKS:
        _PACKS[precision] = tuple(ops.pack_mlp_weights({k: torch.from_numpy(v).to(DEV) for k, v in synth.mlp_state(seed, 2.0, 0.5).items()},
                                                       precision=precision) for seed in (11, 12))
    return _PACKS[precision]


@torch.no_grad()
@pytest.mark.parametrize("nc,ni", [(5, 3), (67, 129), (130, 40), (256, 256)])
@pytest.mark.parametrize("precision", ["f32", "f32x3", "bf16", "auto"])
def test_fused_renderers_sample_what_the_stand_alone_kernel_samples(precision, nc, ni):
    """z_fine of the fused renderer == crnerf_sample_pdf_merge_f32 on the renderer's own weights_coarse, bit for bit, at the multi-chunk sizes
    (the suite holds this at (64, 128)): f32 / bf16 run sample_pdf_pair, f32x3 / auto sample_pdf_wave.  Depths come in as a tensor (no
    linspace table involved), u per ray and unsorted.  "auto": whichever core rendered a ray wrote both its weights_coarse and its z_fine, so
    every ray is compared on the weights returned."""
    n_rays = 5
    g = RC.generator(nc, ni, 23)
    rays = torch.from_numpy(synth.rays(n_rays, seed=3)).to(DEV)
    zc = D(RC.depths(n_rays, nc, g))
    u = D(torch.rand(n_rays, ni, generator=g))
    pc, pf = packs(precision)
    out = ops.render_rays(pc, pf, rays, nc, ni, z_coarse=zc, u=u, want_z_fine=True, precision=precision)
    assert bool(torch.isfinite(out["weights_coarse"]).all())
    assert torch.equal(out["z_fine"], ops.sample_pdf_merge(zc, out["weights_coarse"], ni, u=u))


@torch.no_grad()
@pytest.mark.parametrize("nc,ni", [(67, 129), (256, 256)])
@pytest.mark.parametrize("family", ["onehot", "blocks", "zero"])
def test_pair_sampler_on_adversarial_weights(family, nc, ni):
    """No MLP produces these weights; crnerf_render_rays_bf16_fine takes weights_coarse as an INPUT and is the one entry point that can push
    them through sample_pdf_pair / merge_sort_pair."""
    zc, w, u = RC.sample_case(family, nc, ni)
    rays = torch.from_numpy(synth.rays(RC.R, seed=4)).to(DEV)
    out = ops.render_rays_bf16_fine(packs("bf16")[1], rays, D(w), nc, ni, z_coarse=D(zc), u=D(u), want_z_fine=True)
    assert torch.equal(out["z_fine"], ops.sample_pdf_merge(D(zc), D(w), ni, u=D(u)))


# ------------------------------------------------------------------ compositing at its edges
@torch.no_grad()
@pytest.mark.parametrize("n", RC.COMPOSITE_N)
@pytest.mark.parametrize("kind", RC.COMPOSITE_KINDS)
def test_composite_edges_vs_float64(kind, n):
    """ops.composite against oracle.cpu_ref.composite in float64.  Tolerances: twice the fp32 CPU oracle's own error on these inputs
    (_ray_cases.COMPOSITE_ORACLE_ERR: at most 6.1e-7 / 6.3e-7 / 8.1e-7 on weights / feature / depth, on `thin`), floored at the suite's
    2e-6 / 3e-6 / 1e-5 -- the floors are the larger on every kind.  What must be 0 is asserted as 0."""
    case = RC.composite_case(kind, n)
    ref = RC.composite_ref64(case)
    got = dict(zip(("weights", "feature", "depth"), (t.cpu() for t in ops.composite(D(case["raw"]), D(case["z"]), D(case["noise"]), case["noise_std"]))))
    tol = RC.composite_tolerances(kind)
    err = {k: float((got[k].double() - ref[k]).abs().max()) for k in tol}
    print("composite %-9s N = %3d: %s (allowed %s)" % (kind, n, {k: "%.3g" % v for k, v in err.items()}, {k: "%.3g" % v for k, v in tol.items()}))
    for k in tol:
        assert bool(torch.isfinite(got[k]).all()) and err[k] <= tol[k], (k, err[k], tol[k])
    assert bool((got["weights"][case["zero_weight"]] == 0).all())
    if kind == "saturated":
        assert float((got["weights"].double().sum(1) - 1).abs().max()) <= 1e-6
    if kind == "empty":
        assert bool((got["feature"] == 0).all()) and bool((got["depth"] == 0).all())


@pytest.mark.parametrize("n", RC.COMPOSITE_BACKWARD_N)
@pytest.mark.parametrize("kind", RC.COMPOSITE_KINDS)
def test_composite_backward_edges_vs_float64_autograd(kind, n):
    """ops.composite_backward (d_depth and d_weights present) against float64 autograd through the oracle.  Tolerance: twice the fp32 autograd
    oracle's error (_ray_cases.COMPOSITE_BACKWARD_ORACLE_ERR: at most 7.8e-7 of max |gradient|), floored at test_composite_backward_vs_autograd_oracle's
    2e-5 * max |gradient| + 1e-6 -- the floor is the larger on every kind.  d_sigma is exactly 0 where sigma + noise <= 0 (0 included: relu's
    gradient at 0 is 0, the kernel tests `sig > 0`), where alpha saturated (the factor 1 - alpha is 0) and behind it (T is 0)."""
    case = RC.composite_case(kind, n)
    ref = RC.composite_backward_ref(case)
    gf, gd, gw = RC.backward_upstream(case)
    with torch.no_grad():
        got = ops.composite_backward(D(case["raw"]), D(case["z"]), D(gf), D(gd), D(gw), noise=D(case["noise"]), noise_std=case["noise_std"]).cpu()
    err, tol = float((got.double() - ref).abs().max()), RC.composite_backward_tolerance(kind, ref)
    print("composite backward %-9s N = %3d: %.3g (allowed %.3g, max |gradient| %.3g)" % (kind, n, err, tol, float(ref.abs().max())))
    assert bool(torch.isfinite(got).all()) and err <= tol, (err, tol)
    assert bool((got[..., 64][case["zero_dsigma"]] == 0).all())

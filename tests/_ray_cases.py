"""Shared inputs and float64 references for the per-ray steps every renderer ends its coarse pass with: sample_pdf, the z merge and
compositing (csrc/ray_ops.h for one wave per ray, csrc/pair_ops.h for two).  A plain helper module: tests/test_ray_edges_host.py checks the
fp32 CPU oracle against these references (no GPU), tests/test_gpu_ray_edges.py checks the kernels.

sample_pdf
----------
ref_sample_pdf64() is oracle.cpu_ref.sample_pdf evaluated in float64 on the fp32 inputs.  Besides the depths it returns, per sample, the
float64 cdf gap of the bin the sample fell in, that bin's width and the distance from u to the nearest cdf knot.  A sample is PINNED when
    (gap >= 1e-3  or  gap <= 5e-6)  and  its u is at least 2e-6 away from every knot:
a gap <= 5e-6 is clearly on the `denom < eps -> denom = 1` branch (rendering.py:41-42), where the sample sits within 1e-5 bin widths of the
bin's left end; gaps in between divide by something close to eps = 1e-5 or switch formula on a 1-ulp change of the cdf.  Pinned samples obey
    |z - z64| <= width * K * 2^-23 / max(gap, 1e-3) + 4 ulp(z)          (gap <= 5e-6: the first term is width * 2e-5)
Everything else gets the "stays inside the interval the reference put it in" check of test_gpu_parity.assert_depths.  Every generated case
must have a pinned share of at least MIN_PINNED_SHARE, so the mask cannot hide a failure.

K, measured: the fp32 CPU oracle against the float64 reference over all FAMILIES x SHAPES at R = 16 (test_ray_edges_host.py prints it):
    smallest K that covers the oracle's pinned error          1.16  (`surface` at (65, 65): gap 2e-3, bin width 0.07)
    K_ORACLE (asserted on the oracle; the above, rounded up)  1.2
    K_KERNEL = 4 * K_ORACLE                                   4.8
The kernels get 4x: their sum of the pdf weights is lane-strided where ATen's is pairwise, and either adds up to ~ n * 2^-24 relative to
every knot.  The oracle's largest pinned error was 5.9e-6 (`surface` at (33, 63)); outside `surface` and `smooth` it stayed below 9e-7.

compositing
-----------
composite_case() builds the edge inputs (saturated alpha, sigma + noise <= 0 with exact zeros, repeated depths, 257 thin samples, empty space),
composite_ref64() is oracle.cpu_ref.composite in float64 and composite_backward_ref() autograd through it.  COMPOSITE_ORACLE_ERR /
COMPOSITE_BACKWARD_ORACLE_ERR record the fp32 oracle's largest error against float64 on these inputs; composite_tolerances() /
composite_backward_tolerance() give a kernel twice that, floored at the bounds the suite already uses.
"""
import torch

from oracle import cpu_ref as O

# ------------------------------------------------------------------ sample_pdf
R = 16
SHAPES = [(3, 5), (4, 1), (33, 63), (64, 64), (65, 65), (66, 128), (67, 129), (130, 40), (256, 256)]
FAMILIES = ("smooth", "zero", "onehot", "blocks", "surface")
MIN_PINNED_SHARE = 0.95
K_ORACLE = 1.2
K_KERNEL = 4.0 * K_ORACLE
GAP_WELL, GAP_FLAT, KNOT_CLEAR = 1e-3, 5e-6, 2e-6
LOOSE = 3e-5          # assert_depths' slack on the interval check


def generator(*key):
    g = torch.Generator()
    g.manual_seed(sum(int(k) * m for k, m in zip(key, (1000003, 10007, 101, 1))))
    return g


def depths(n_rays, nc, g):
    """near * (1 - s) + far * s, near in [0.1, 0.6], far = near + 2..5."""
    near = 0.1 + 0.5 * torch.rand(n_rays, 1, generator=g)
    far = near + 2.0 + 3.0 * torch.rand(n_rays, 1, generator=g)
    s = torch.linspace(0, 1, nc)
    return (near * (1 - s) + far * s).contiguous()


def weights(family, n_rays, nc, g):
    """Coarse weights [n_rays, nc] of one family.  The sampler reads the interior nc - 2 only: the two end weights are random junk, so a
    kernel that let them into the pdf would miss the reference."""
    m = nc - 2
    if family == "smooth":
        w = torch.rand(n_rays, m, generator=g) + 0.05
        w = w / w.sum(1, keepdim=True)
    elif family == "zero":
        w = torch.zeros(n_rays, m)
    elif family == "onehot":
        w = torch.zeros(n_rays, m)
        w[torch.arange(n_rays), torch.randint(0, m, (n_rays,), generator=g)] = 1.0
    elif family == "blocks":      # about half the bins exactly 0, total mass 4: an empty bin's pdf is 1e-5 / 4 = 2.5e-6, clear of eps
        keep = torch.rand(n_rays, m, generator=g) < 0.5
        keep[torch.arange(n_rays), torch.randint(0, m, (n_rays,), generator=g)] = True
        w = (torch.rand(n_rays, m, generator=g) + 0.5) * keep
        w = w * (4.0 / w.sum(1, keepdim=True))
    elif family == "surface":     # empty space, then a surface: 0.5^k from a random index on
        start = torch.randint(0, m, (n_rays, 1), generator=g)
        k = torch.arange(m)[None, :] - start
        w = torch.where(k >= 0, torch.pow(torch.tensor(0.5), k.clamp_min(0).float()), torch.zeros(()))
    else:
        raise ValueError(family)
    ends = torch.rand(n_rays, 2, generator=g)
    return torch.cat((ends[:, :1], w.float(), ends[:, 1:]), 1).contiguous()


def sample_case(family, nc, ni, n_rays=R):
    """(z_coarse [R,nc], weights [R,nc], u [R,ni]) -- fp32 CPU tensors; u is per ray and unsorted."""
    g = generator(FAMILIES.index(family), nc, ni, n_rays)
    return depths(n_rays, nc, g), weights(family, n_rays, nc, g), torch.rand(n_rays, ni, generator=g)


def midpoints(z_coarse):
    return 0.5 * (z_coarse[:, :-1] + z_coarse[:, 1:])


def ref_sample_pdf64(z_coarse, weights, u):
    """oracle.cpu_ref.sample_pdf in float64 on midpoints(z_coarse) and weights[:, 1:-1].  Returns (z, gap, width, knot), each [R, Ni] float64:
    the depths, the cdf gap and the width of the bin every sample fell in, and the distance from u to the nearest cdf knot."""
    zc, w, u = (torch.as_tensor(t).detach().cpu().double() for t in (z_coarse, weights, u))
    if u.dim() == 1:
        u = u.expand(zc.shape[0], u.shape[0])
    u = u.contiguous()
    mid, wi = midpoints(zc), w[:, 1:-1]
    m = wi.shape[1]
    z = O.sample_pdf(mid, wi, u.shape[1], u=u)
    pdf = (wi + 1e-5) / (wi + 1e-5).sum(1, keepdim=True)
    cdf = torch.cat((torch.zeros(zc.shape[0], 1, dtype=torch.float64), torch.cumsum(pdf, -1)), -1)
    idx = torch.searchsorted(cdf, u, right=True)
    lo, hi = (idx - 1).clamp_min(0), idx.clamp_max(m)
    gap = cdf.gather(1, hi) - cdf.gather(1, lo)
    width = (mid.gather(1, hi) - mid.gather(1, lo)).abs()
    knot = (u[:, :, None] - cdf[:, None, :]).abs().amin(-1)
    return z, gap, width, knot


def ulp32(x):
    """Spacing of fp32 at |x| (float64 tensor in, float64 out)."""
    e = torch.floor(torch.log2(x.abs().clamp_min(2.0 ** -126)))
    return torch.pow(torch.tensor(2.0, dtype=torch.float64), e - 23)


def pinned_mask(gap, knot):
    return ((gap >= GAP_WELL) | (gap <= GAP_FLAT)) & (knot >= KNOT_CLEAR)


def pinned_bound(z64, gap, width, k):
    first = torch.where(gap <= GAP_FLAT, width * 2e-5, width * k * 2.0 ** -23 / gap.clamp_min(GAP_WELL))
    return first + 4 * ulp32(z64)


def check_samples(z, z_coarse, weights, u, k, min_share=None, what=""):
    """Hold fp32 samples `z` [R,Ni] to ref_sample_pdf64: the pinned bound with constant `k` on pinned samples, the reference's interval on the
    rest.  Returns {"share", "k_needed", "max_err"} (pinned share; the smallest k that would have covered the pinned samples; their largest
    error)."""
    z = torch.as_tensor(z).detach().cpu().double()
    z64, gap, width, knot = ref_sample_pdf64(z_coarse, weights, u)
    err = (z - z64).abs()
    pin = pinned_mask(gap, knot)
    share = float(pin.double().mean())
    scaled = pin & (gap >= GAP_WELL) & (width > 0)
    over = (err - 4 * ulp32(z64)).clamp_min(0) * gap.clamp_min(GAP_WELL) / (width.clamp_min(1e-30) * 2.0 ** -23)
    stats = {"share": share, "k_needed": float(over[scaled].max()) if bool(scaled.any()) else 0.0,
             "max_err": float(err[pin].max()) if bool(pin.any()) else 0.0}
    assert bool(torch.isfinite(z).all()), what
    if min_share is not None:
        assert share >= min_share, "%s: only %.3f of the samples are pinned" % (what, share)
    bad = pin & (err > pinned_bound(z64, gap, width, k))
    if bool(bad.any()):
        r, i = (int(v) for v in bad.nonzero()[0])
        raise AssertionError("%s: %d pinned samples miss the bound (k needed %.3g, allowed %.3g); first at ray %d sample %d: got %.9g want %.9g, "
                             "gap %.3g width %.3g" % (what, int(bad.sum()), stats["k_needed"], k, r, i, float(z[r, i]), float(z64[r, i]),
                                                      float(gap[r, i]), float(width[r, i])))
    loose = ~pin & (err > width + LOOSE)
    assert not bool(loose.any()), "%s: %d ill-conditioned samples left the interval the reference put them in" % (what, int(loose.sum()))
    return stats


def tied_depths(n_rays, nc, g):
    """Ascending coarse depths in runs of 2-5 equal values: zero-width bins, whose samples equal a coarse depth exactly."""
    base = depths(n_rays, nc, g)
    runs = torch.randint(2, 6, (n_rays, nc), generator=g)
    starts = torch.cumsum(runs, 1) - runs                       # first index of every run, while < nc
    idx = torch.zeros(n_rays, nc, dtype=torch.long)
    for r in range(n_rays):
        s = starts[r][starts[r] < nc]
        owner = torch.searchsorted(s, torch.arange(nc), right=True) - 1
        idx[r] = s[owner]
    return base.gather(1, idx).contiguous()


def shuffle_rows(t, g):
    perm = torch.rand(t.shape, generator=g).argsort(1)
    return t.gather(1, perm).contiguous()


# ------------------------------------------------------------------ compositing
COMPOSITE_R = 9
COMPOSITE_N = [1, 2, 31, 32, 33, 64, 65, 128, 129, 256, 257]
COMPOSITE_BACKWARD_N = [1, 33, 65, 129, 257]
COMPOSITE_KINDS = ("saturated", "clamped", "flat", "thin", "empty")
FLOORS = {"weights": 2e-6, "feature": 3e-6, "depth": 1e-5}      # test_composite_golden / test_composite_ragged_vs_oracle
BACKWARD_FLOOR = 2e-5                                            # relative to max |gradient|, + 1e-6: test_composite_backward_vs_autograd_oracle
# the fp32 CPU oracle against itself in float64, largest over COMPOSITE_N (test_ray_edges_host.py asserts these and prints what it measured)
COMPOSITE_ORACLE_ERR = {
    "saturated": {"weights": 6.9e-8, "feature": 2.2e-7, "depth": 2.0e-7},
    "clamped": {"weights": 5.2e-8, "feature": 1.7e-7, "depth": 2.4e-7},
    "flat": {"weights": 5.3e-8, "feature": 2.2e-7, "depth": 9.6e-8},
    "thin": {"weights": 6.1e-7, "feature": 6.3e-7, "depth": 8.1e-7},       # 256 factors (1 - alpha), each rounded to fp32 before the product
    "empty": {"weights": 0.0, "feature": 0.0, "depth": 0.0},
}
# fp32 autograd through the oracle against float64 autograd, max |d| / max |gradient|, largest over COMPOSITE_BACKWARD_N
COMPOSITE_BACKWARD_ORACLE_ERR = {"saturated": 1.7e-7, "clamped": 4.4e-7, "flat": 9.0e-8, "thin": 7.8e-7, "empty": 0.0}
# twice any of these is below the floors, so the floors are what the kernels are held to on every kind


def composite_case(kind, n, n_rays=COMPOSITE_R):
    """fp32 CPU inputs of ops.composite / oracle.cpu_ref.composite: {"raw" [R,n,65], "z" [R,n], "noise" [R,n] or None, "noise_std"} plus what
    the kind promises: "zero_weight" (bool [R,n]: the weight there is exactly 0) and "zero_dsigma" (bool [R,n]: d_sigma there is exactly 0)."""
    g = generator(COMPOSITE_KINDS.index(kind), n, n_rays, 77)
    raw = torch.rand(n_rays, n, 65, generator=g)
    z = depths(n_rays, n, g)
    noise, noise_std = None, 0.0
    zero_w = torch.zeros(n_rays, n, dtype=torch.bool)
    zero_ds = torch.zeros(n_rays, n, dtype=torch.bool)
    rows = torch.arange(n_rays)
    if kind == "saturated":       # one opaque sample at a random index: alpha == 1 there, T == 0 behind it
        raw[..., 64] = 2.0 * torch.rand(n_rays, n, generator=g)
        k = torch.randint(0, n, (n_rays,), generator=g)
        raw[rows, k, 64] = 1e4
        zero_w = torch.arange(n)[None, :] > k[:, None]
        zero_ds = torch.arange(n)[None, :] >= k[:, None]
    elif kind == "clamped":       # sigma + noise * noise_std spread over [-5, 5] on a 2^-10 grid (the sum is exact in fp32 and float64 alike), exact zeros
        noise_std = 0.5
        target = torch.round((10.0 * torch.rand(n_rays, n, generator=g) - 5.0) * 1024) / 1024
        target[torch.rand(n_rays, n, generator=g) < 0.15] = 0.0
        target[rows, torch.randint(0, n, (n_rays,), generator=g)] = 0.0
        sigma = torch.round((6.0 * torch.rand(n_rays, n, generator=g) - 3.0) * 1024) / 1024
        raw[..., 64] = sigma
        noise = ((target - sigma) * 2.0).contiguous()
        assert torch.equal(sigma + noise * noise_std, target)
        zero_w = target <= 0
        zero_ds = target <= 0
    elif kind == "flat":          # runs of equal depths: delta == 0, alpha == 0, weight == 0 on all but the last sample of a run
        raw[..., 64] = 20.0 * torch.rand(n_rays, n, generator=g)
        z = tied_depths(n_rays, n, g)
        zero_w[:, :-1] = z[:, 1:] == z[:, :-1]
    elif kind == "thin":          # alpha ~ 1e-4 per sample: after 257 of them T is still ~0.97, carried by the fp64 prefix product
        delta = 3.0 / max(n - 1, 1)                              # the depths span 2..5
        raw[..., 64] = 1e-4 / delta * (0.5 + torch.rand(n_rays, n, generator=g))
    elif kind == "empty":
        raw[..., 64] = 0.0
        zero_w[:] = True
        zero_ds[:] = True
    else:
        raise ValueError(kind)
    return {"raw": raw.contiguous(), "z": z, "noise": noise, "noise_std": noise_std, "zero_weight": zero_w, "zero_dsigma": zero_ds}


def _as(case, dtype):
    return (case["raw"].to(dtype), case["z"].to(dtype), None if case["noise"] is None else case["noise"].to(dtype), case["noise_std"])


def composite_ref64(case):
    """oracle.cpu_ref.composite in float64: {"weights", "feature", "depth"}."""
    return dict(zip(("weights", "feature", "depth"), O.composite(*_as(case, torch.float64))))


def composite_oracle32(case):
    return dict(zip(("weights", "feature", "depth"), O.composite(*_as(case, torch.float32))))


def composite_tolerances(kind):
    return {k: max(2.0 * COMPOSITE_ORACLE_ERR[kind][k], FLOORS[k]) for k in FLOORS}


def backward_upstream(case):
    """(d_feature [R,64], d_depth [R], d_weights [R,n]), fp32, seeded by the case's shape."""
    n_rays, n = case["z"].shape
    g = generator(n_rays, n, 5, 5)
    return torch.randn(n_rays, 64, generator=g), torch.randn(n_rays, generator=g), torch.randn(n_rays, n, generator=g)


def composite_backward_ref(case, dtype=torch.float64):
    """d loss / d raw [R,n,65] by autograd through oracle.cpu_ref.composite in `dtype`, loss = <feature, gf> + <depth, gd> + <weights, gw>."""
    raw, z, noise, noise_std = _as(case, dtype)
    gf, gd, gw = (t.to(dtype) for t in backward_upstream(case))
    raw = raw.clone().requires_grad_(True)
    w, f, d = O.composite(raw, z, noise, noise_std)
    ((f * gf).sum() + (d * gd).sum() + (w * gw).sum()).backward()
    return raw.grad


def composite_backward_tolerance(kind, ref):
    return max(2.0 * COMPOSITE_BACKWARD_ORACLE_ERR[kind], BACKWARD_FLOOR) * (float(ref.abs().max()) + 1e-6) + 1e-6


"""Where is the geometry?  The density of a trained NeRF_sigma at points that do not come from rays: a point list, or the nodes of a grid --
what mesh extraction (scipy / skimage / PyMCubes take the grid as it is), occupancy visualisation and point-cloud export start from.

    sigma_points(model, xyz)                      [n]           sigma at xyz [n,3]
    sigma_grid(model, xs, ys, zs)                 [nz, ny, nx]  sigma at (xs[ix], ys[iy], zs[iz]); the axes need not be uniform
    density_grid(model, lo, hi, resolution)       a DensityGrid: sigma on torch.linspace axes, and .occupied(threshold) -> [m,3] point cloud

One launch each (include/crnerf_geometry.h): the coordinates are all that is read, the embedding is built in registers and the weight stream is
walked up to the sigma head only.  `model` is a NeRF_sigma; its packed_weights(precision) is the pack.  precision "f32" or "bf16".
Inference only; GPU tensors only: like every op of the package there is no CPU fallback.

Domain: |coordinate| < 64.  Below it the kernels' embedding is the routine the stand-alone posenc uses (which switches to ocml's sincosf there);
the fused routine degrades beyond 200.  sigma_grid and density_grid refuse an axis or a bound outside the domain (the axes are small: the check
reads them back); sigma_points does not check its points.
"""
import torch

from . import ops

DOMAIN = 64.0      # |coordinate| must stay below it


class DensityGrid:
    """sigma [nz, ny, nx] and the axes it was sampled on (device tensors)."""
    __slots__ = ("sigma", "xs", "ys", "zs")

    def __init__(self, sigma, xs, ys, zs):
        self.sigma, self.xs, self.ys, self.zs = sigma, xs, ys, zs

    @torch.no_grad()
    def occupied(self, threshold):
        """[m,3]: the scene coordinates (x, y, z) of the nodes with sigma > threshold, in the grid's memory order (z slowest)."""
        iz, iy, ix = torch.nonzero(self.sigma > threshold, as_tuple=True)
        return torch.stack((self.xs[ix], self.ys[iy], self.zs[iz]), dim=1)


def _check_axis(t, name):
    """Rank, then domain -- wherever the axis lives: the refusal needs no device."""
    ops._sigma_input(t, name, "sigma_grid", on_device=False)
    if t.numel() > 0:
        worst = float(t.abs().max())
        if not worst < DOMAIN:          # (a NaN is refused too)
            raise ValueError("crnerf_amd.geometry: the axis %s reaches |v| = %g; the density query is defined for |v| < %g" % (name, worst, DOMAIN))


@torch.no_grad()
def sigma_points(model, xyz, precision="f32"):
    """sigma [n] at xyz [n,3] (float32, contiguous, on the GPU).  Domain |coordinate| < 64: documented, not checked."""
    name = ops._sigma_query_core(precision, "sigma_points")
    ops._sigma_input(xyz, "xyz", "sigma_points", points=True)
    return ops.sigma_points(model.packed_weights(name), xyz, precision=precision)


@torch.no_grad()
def sigma_grid(model, xs, ys, zs, precision="f32", out=None):
    """sigma [nz, ny, nx] at (xs[ix], ys[iy], zs[iz]); the axes are 1-D float32 device tensors with |v| < 64 (ValueError otherwise).  out=: see
    ops.sigma_grid."""
    name = ops._sigma_query_core(precision, "sigma_grid")
    for t, n in ((xs, "xs"), (ys, "ys"), (zs, "zs")):
        _check_axis(t, n)
    for t, n in ((xs, "xs"), (ys, "ys"), (zs, "zs")):      # float32, contiguous, on the device: before the model is asked for its pack
        ops._sigma_input(t, n, "sigma_grid")
    return ops.sigma_grid(model.packed_weights(name), xs, ys, zs, precision=precision, out=out)


@torch.no_grad()
def density_grid(model, lo, hi, resolution, precision="f32"):
    """The density on the box [lo, hi] (3-sequences of floats, scene coordinates): axis a is torch.linspace(lo[a], hi[a], n[a]) with
    n = resolution (an int, or (nx, ny, nz)).  Returns a DensityGrid."""
    name = ops._sigma_query_core(precision, "density_grid")
    lo, hi = [float(v) for v in lo], [float(v) for v in hi]
    n = [int(resolution)] * 3 if isinstance(resolution, int) else [int(v) for v in resolution]
    if len(lo) != 3 or len(hi) != 3 or len(n) != 3:
        raise ValueError("crnerf_amd.geometry: density_grid expects lo and hi as 3-sequences and resolution as an int or (nx, ny, nz)")
    if min(n) < 1:
        raise ValueError("crnerf_amd.geometry: density_grid: resolution must be positive, got %s" % (n,))
    for v in lo + hi:
        if not abs(v) < DOMAIN:
            raise ValueError("crnerf_amd.geometry: density_grid: the bound %g is outside |v| < %g, the domain of the density query" % (v, DOMAIN))
    pack = model.packed_weights(name)
    dev = pack.device
    xs, ys, zs = (torch.linspace(lo[a], hi[a], n[a], dtype=torch.float32, device=dev) for a in range(3))
    return DensityGrid(ops.sigma_grid(pack, xs, ys, zs, precision=precision), xs, ys, zs)

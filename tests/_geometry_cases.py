"""Inputs of tests/test_gpu_geometry.py (the density query, include/crnerf_geometry.h): the two networks, their packs, the grids and the point lists
the grids stand for, and the composed route's answer -- ops.posenc + ops.mlp_forward(sigma_only=True), what a caller had to run before.  Everything
is built once per process and never modified.

The axes are non-uniform and different per axis (sorted seeded uniforms in [-3, 3], [-2, 2.5], [-1, 4]) and nx, ny, nz are distinct wherever the
shape allows it: an index decomposition with two axes swapped cannot pass."""
import numpy as np
import torch

import crnerf_amd.synth as synth
from crnerf_amd import ops

DEV = "cuda:0"
STATES = {21: synth.mlp_state(21, 2.0), 22: synth.mlp_state(22, 2.0)}
RANGES = ((-3.0, 3.0), (-2.0, 2.5), (-1.0, 4.0))          # x, y, z

# (nx, ny, nz): points -- what it exercises
SMALL_SHAPES = [(5, 3, 2),        # 30: under one tile group
                (16, 8, 1),       # 128: exactly one fp32 workgroup iteration
                (129, 1, 1),      # 129: one point into the next group
                (17, 9, 7),       # 1,071: ragged
                (1, 1, 300)]      # 300: a column
# 132,500 points: five sweeps of a 256-workgroup grid on fp32 (128 points an iteration), three on bf16 (256), so the pair core walks the ring
# phases 0, 2, 0; the last sweep is partly empty
LARGE_SHAPE = (53, 50, 50)
SHAPES = SMALL_SHAPES + [LARGE_SHAPE]


def axes_cpu(shape):
    """(xs, ys, zs) float32 CPU tensors for a shape; the seed is the shape."""
    rng = np.random.default_rng(list(shape))
    return tuple(torch.from_numpy(np.sort(rng.uniform(lo, hi, n)).astype(np.float32)) for n, (lo, hi) in zip(shape, RANGES))


def points_cpu(shape):
    """[nx * ny * nz, 3] (x, y, z), x fastest: the point list the grid stands for, from meshgrid -- not from the index arithmetic under test."""
    xs, ys, zs = axes_cpu(shape)
    Z, Y, X = torch.meshgrid(zs, ys, xs, indexing="ij")          # each [nz, ny, nx]
    return torch.stack((X, Y, Z), dim=-1).reshape(-1, 3).contiguous()


_CACHE = {}


def _once(key, build):
    if key not in _CACHE:
        _CACHE[key] = build()
    return _CACHE[key]


def pack(seed, precision):
    return _once(("pack", seed, precision),
                 lambda: ops.pack_mlp_weights({k: torch.from_numpy(v).to(DEV) for k, v in STATES[seed].items()}, precision=precision))


def axes(shape):
    return _once(("axes", shape), lambda: tuple(t.to(DEV) for t in axes_cpu(shape)))


def points(shape):
    return _once(("points", shape), lambda: points_cpu(shape).to(DEV))


@torch.no_grad()
def composed(seed, shape, precision):
    """sigma [n] by the route a caller had before: the embedded rows through HBM, then the whole MLP with sigma_only."""
    return _once(("composed", seed, shape, precision),
                 lambda: ops.mlp_forward(pack(seed, precision), ops.posenc(points(shape), 15), sigma_only=True, precision=precision)[:, 0].clone())

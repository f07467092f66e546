"""Inputs of tests/test_gpu_point_features.py (the point-feature query, csrc/crnerf_point_features.h): the nets and packs of _geometry_cases, point
lists from its ranges, a view direction per point, the composed route's answer -- ops.posenc twice, torch.cat, ops.mlp_forward: what a caller had to
run before -- and the oracle's.  Everything is built once per process and never modified.

Directions: seeded unit vectors, behind the three rows (0,0,0) -- what Mesh.colorize hands over for a zero normal --, (1,0,0) and (0,0,-1)."""
import numpy as np
import torch

from crnerf_amd import ops
from oracle import cpu_ref as O

import _geometry_cases as G

# n: what it exercises
SMALL_N = [30,        # under one tile group
           128,       # exactly one fp32 workgroup iteration (8 waves x 16 points)
           129,       # one point into the next
           257,       # one point past a bf16 workgroup iteration (eight 32-point tiles)
           1071]      # ragged
# five sweeps of a 256-workgroup grid on fp32 (128 points an iteration), three on bf16 (256): every workgroup iterates, the last sweep is partly empty
LARGE_N = 132500
FIXED_DIRS = [(0.0, 0.0, 0.0), (1.0, 0.0, 0.0), (0.0, 0.0, -1.0)]


def points_cpu(n):
    """[n,3] seeded uniforms in _geometry_cases.RANGES; the seed is n."""
    rng = np.random.default_rng([n, 1])
    return torch.from_numpy(np.stack([rng.uniform(lo, hi, n) for lo, hi in G.RANGES], axis=1).astype(np.float32)).contiguous()


def dirs_cpu(n):
    """[n,3]: FIXED_DIRS, then seeded unit vectors."""
    rng = np.random.default_rng([n, 2])
    d = rng.standard_normal((n, 3))
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    d[:len(FIXED_DIRS)] = np.asarray(FIXED_DIRS, dtype=np.float32)
    return torch.from_numpy(d).contiguous()


def points(n):
    return G._once(("pf_points", n), lambda: points_cpu(n).to(G.DEV))


def dirs(n):
    return G._once(("pf_dirs", n), lambda: dirs_cpu(n).to(G.DEV))


@torch.no_grad()
def composed_at(pack, xyz, dirs_, precision):
    """[n,65] by the route a caller had before: both embeddings and the cat through HBM, then the module entry."""
    return ops.mlp_forward(pack, torch.cat((ops.posenc(xyz, 15), ops.posenc(dirs_, 4)), dim=1), precision=precision)


def composed(seed, n, precision):
    return G._once(("pf_composed", seed, n, precision), lambda: composed_at(G.pack(seed, precision), points(n), dirs(n), precision).clone())


@torch.no_grad()
def oracle(seed, n, precision):
    """[n,65] float32 on the CPU: O.mlp_forward (or its bf16 restatement) on O.posenc."""
    fwd = O.mlp_forward if precision == "f32" else O.mlp_forward_bf16
    return G._once(("pf_oracle", seed, n, precision),
                   lambda: fwd(O.to_torch(G.STATES[seed]), torch.cat((O.posenc(points_cpu(n), 15), O.posenc(dirs_cpu(n), 4)), dim=1)))

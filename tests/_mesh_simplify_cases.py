"""The rules of csrc/crnerf_mesh_simplify.h restated in NumPy, and the hand cases of the simplification tests (tests/test_mesh_simplify_host.py,
tests/test_gpu_mesh_simplify.py).  Test infrastructure: written from the rules, not from csrc/mesh_simplify.hip -- np.unique and np.minimum.at
stand where the kernels have a leader table, a hash table and atomics; the integer sums are np.add.at into int64; the position, normal and colour
formulas are spelled in float32 / float64 operation by operation, as the header states them.

cluster_ref(vertices, faces, lo, cell, n, normals=None, colors=None)
    -> (vertices' float32, faces' int32, normals' float32 | None, colors' float32 | None, vertex_cluster int32)
sums_ref(...) -> the members, position, normal and colour sums per cluster (int64), for the tests that look at the sums themselves
grid_of(vertices, cell, lo=None, hi=None) -> (lo, cell, n): what crnerf_amd.geometry.Mesh.simplify hands to the library"""
import math

import numpy as np

FIXED = np.float32(1048576.0)      # 2^20


def cells_ref(vertices, lo, cell, n):
    """(s [V,3] float32, clamped; c [V,3] int64; key [V] int64) by "Cell of a vertex"."""
    v = np.asarray(vertices, dtype=np.float32).reshape(-1, 3)
    lo, cell = np.asarray(lo, dtype=np.float32), np.asarray(cell, dtype=np.float32)
    n = np.asarray(n, dtype=np.int64)
    inv = (np.float32(1.0) / cell).astype(np.float32)
    s = ((v - lo).astype(np.float32) * inv).astype(np.float32)      # two float32 operations, each rounded
    s = np.minimum(np.maximum(s, np.float32(0.0)), n.astype(np.float32))
    c = np.minimum(s.astype(np.int64), n - 1)                       # (int) truncates; s >= 0
    key = c[:, 0] + n[0] * (c[:, 1] + n[1] * c[:, 2])
    return s, c, key


def _fixed(x, lo, hi):
    """(int) rintf(clamp(x, lo, hi) * 2^20) per element."""
    x = np.minimum(np.maximum(np.asarray(x, dtype=np.float32), np.float32(lo)), np.float32(hi))
    return np.rint((x * FIXED).astype(np.float32)).astype(np.int64)


def sums_ref(vertices, lo, cell, n, normals=None, colors=None):
    """vertex_cluster and, per cluster: its cell c [V',3], members m, position sums S [V',3], normal sums, colour sums (int64; None when not given)."""
    s, c, key = cells_ref(vertices, lo, cell, n)
    V = len(key)
    _, first, inverse = np.unique(key, return_index=True, return_inverse=True)      # first: the smallest member id of every occupied cell
    order = np.argsort(first, kind="stable")                                        # cluster ids ascend in the leader's id
    rank = np.empty(len(order), dtype=np.int64)
    rank[order] = np.arange(len(order))
    vc = rank[inverse.reshape(-1)] if V else np.zeros(0, np.int64)
    K = len(order)
    r = np.floor(((s - c.astype(np.float32)).astype(np.float32) * FIXED).astype(np.float32)).astype(np.int64)
    assert V == 0 or (r.min() >= 0 and r.max() <= 2 ** 20)
    m = np.bincount(vc, minlength=K).astype(np.int64)
    S = np.zeros((K, 3), np.int64)
    np.add.at(S, vc, r)
    cc = np.zeros((K, 3), np.int64)
    cc[vc] = c                                                                      # every member of a cluster has the same cell
    N = C = None
    if normals is not None:
        N = np.zeros((K, 3), np.int64)
        np.add.at(N, vc, _fixed(np.asarray(normals).reshape(-1, 3), -1.0, 1.0))
    if colors is not None:
        C = np.zeros((K, 3), np.int64)
        np.add.at(C, vc, _fixed(np.asarray(colors).reshape(-1, 3), 0.0, 1.0))
    return vc.astype(np.int32), cc, m, S, N, C


def cluster_ref(vertices, faces, lo, cell, n, normals=None, colors=None):
    lo32, cell32 = np.asarray(lo, dtype=np.float32), np.asarray(cell, dtype=np.float32)
    vc, cc, m, S, N, C = sums_ref(vertices, lo32, cell32, n, normals, colors)
    V, K = len(vc), len(m)
    scale = (m.astype(np.float64) * 1048576.0)[:, None]
    pos = (lo32.astype(np.float64) + (cc.astype(np.float64) + S.astype(np.float64) / scale) * cell32.astype(np.float64)).astype(np.float32)
    out_n = out_c = None
    if N is not None:
        x = N.astype(np.float64)
        d = np.sqrt(x[:, 0] * x[:, 0] + x[:, 1] * x[:, 1] + x[:, 2] * x[:, 2])
        zero = (N == 0).all(axis=1)
        out_n = np.zeros((K, 3), np.float32)
        out_n[~zero] = (x[~zero] / d[~zero, None]).astype(np.float32)
    if C is not None:
        out_c = (C.astype(np.float64) / scale).astype(np.float32)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    valid = ((f >= 0) & (f < V)).all(axis=1)
    t = np.full(f.shape, -1, np.int64)
    t[valid] = vc[f[valid]]
    alive = valid & (t[:, 0] != t[:, 1]) & (t[:, 0] != t[:, 2]) & (t[:, 1] != t[:, 2])
    idx = np.nonzero(alive)[0]
    sets = np.sort(t[idx], axis=1)
    _, first = np.unique(sets, axis=0, return_index=True) if len(idx) else (None, np.zeros(0, np.int64))      # the smallest index of every set
    kept = np.sort(idx[first])                                                      # in input order
    out_f = t[kept]
    roll = np.argmin(out_f, axis=1) if len(kept) else np.zeros(0, np.int64)         # the cycle as given, the smallest id first
    out_f = np.stack([out_f[np.arange(len(kept)), (roll + j) % 3] for j in range(3)], axis=1) if len(kept) else np.zeros((0, 3), np.int64)
    return pos.reshape(K, 3), out_f.astype(np.int32).reshape(-1, 3), out_n, out_c, vc


def grid_of(vertices, cell, lo=None, hi=None):
    """(lo, cell, n) as Mesh.simplify works them out: the bounding box where a bound is not given, n_a = max(1, ceil((hi_a - lo_a) / cell_a)) in
    Python floats."""
    v = np.asarray(vertices, dtype=np.float32).reshape(-1, 3)
    cell = [float(cell)] * 3 if np.ndim(cell) == 0 else [float(c) for c in cell]
    lo = [float(x) for x in (v.min(axis=0) if lo is None else lo)]
    hi = [float(x) for x in (v.max(axis=0) if hi is None else hi)]
    return lo, cell, [max(1, math.ceil((hi[a] - lo[a]) / cell[a])) for a in range(3)]


# ---------------------------------------------------------------------------------------------------------------- hand cases
# name -> dict(v, f, lo, cell, n, vc, out_f, and what else the case pins): small enough to check by eye.  Unit cells from the origin unless said.
def _case(v, f, n, vc, out_f, lo=(0.0, 0.0, 0.0), cell=(1.0, 1.0, 1.0), **more):
    return dict(v=np.asarray(v, np.float32).reshape(-1, 3), f=np.asarray(f, np.int32).reshape(-1, 3), lo=lo, cell=cell, n=n,
                vc=np.asarray(vc, np.int32), out_f=np.asarray(out_f, np.int32).reshape(-1, 3), **more)


HAND = {
    # vertices 1 and 4 share cell (1,0,0), 2 and 5 share (0,1,0): the second triangle lands on the first one's clusters with 3 -> a new one
    "two triangles merging": _case(
        [[.5, .5, .5], [1.25, .5, .5], [.5, 1.5, .5], [1.5, 1.5, .5], [1.75, .5, .5], [.5, 1.25, .5]], [[0, 1, 2], [4, 3, 5]], (2, 2, 1),
        [0, 1, 2, 3, 1, 2], [[0, 1, 2], [1, 3, 2]],
        out_v=[[.5, .5, .5], [1.5, .5, .5], [.5, 1.375, .5], [1.5, 1.5, .5]]),
    # the second face has two corners in cell (0,0,0)
    "a face that collapses": _case(
        [[.5, .5, .5], [1.5, .5, .5], [.5, 1.5, .5], [.25, .25, .25]], [[0, 1, 2], [0, 3, 1], [3, 1, 2]], (2, 2, 1),
        [0, 1, 2, 0], [[0, 1, 2]]),
    # two faces of different vertices over the same three cells: the first stays, whatever the second looks like
    "two faces over the same three cells": _case(
        [[.5, .5, .5], [1.5, .5, .5], [.5, 1.5, .5], [.75, .75, .5], [1.75, .25, .5], [.25, 1.75, .5]], [[3, 4, 5], [0, 1, 2]], (2, 2, 1),
        [0, 1, 2, 0, 1, 2], [[0, 1, 2]]),
    # the same set in the opposite orientation: the first stays with ITS cycle, rotated so that the smallest id comes first
    "an opposite pair": _case(
        [[.5, .5, .5], [1.5, .5, .5], [.5, 1.5, .5]], [[2, 1, 0], [0, 1, 2], [1, 0, 2]], (2, 2, 1),
        [0, 1, 2], [[0, 2, 1]]),
    "invalid ids": _case(
        [[.5, .5, .5], [1.5, .5, .5], [.5, 1.5, .5]], [[0, 1, 3], [-1, 1, 2], [0, 1, 2], [2 ** 31 - 1, 0, 1], [0, -2 ** 31, 2]], (2, 2, 1),
        [0, 1, 2], [[0, 1, 2]]),
    # vertex 1 is used by no face: its cluster stays, between the others, in leader order
    "an unreferenced vertex": _case(
        [[.5, .5, .5], [1.5, 1.5, .5], [1.5, .5, .5], [.5, 1.5, .5]], [[0, 2, 3]], (2, 2, 1),
        [0, 1, 2, 3], [[0, 2, 3]]),
    "everything in one cell": _case(
        [[.5, .5, .5], [.25, .5, .5], [.5, .75, .5], [.75, .25, .125]], [[0, 1, 2], [1, 2, 3]], (1, 1, 1),
        [0, 0, 0, 0], np.zeros((0, 3)), out_v=[[.5, .5, .40625]]),
    # cells of 1/8 on a 16^3 grid: every vertex alone; the second face is given with its smallest id last
    "nothing merges": _case(
        [[.3, .3, .3], [1.7, .3, .3], [.3, 1.7, .3], [1.7, 1.7, 1.7]], [[0, 1, 2], [3, 2, 1]], (16, 16, 16),
        [0, 1, 2, 3], [[0, 1, 2], [1, 3, 2]], cell=(.125, .125, .125)),
    "empty": _case(np.zeros((0, 3)), np.zeros((0, 3)), (2, 2, 2), [], np.zeros((0, 3))),
    "no faces": _case([[.5, .5, .5], [1.5, .5, .5], [.75, .5, .5]], np.zeros((0, 3)), (2, 1, 1), [0, 1, 0], np.zeros((0, 3)),
                      out_v=[[.625, .5, .5], [1.5, .5, .5]]),
    # the box is [0,2]^3: vertex 1 lies ON the far x face (s = n: the last cell), 2 beyond it, 3 below the near faces, 4 far outside on every axis
    "the clamp": _case(
        [[1.5, .5, .5], [2.0, .5, .5], [7.0, .5, .5], [-3.0, -.5, .5], [1e30, 1e30, -1e30]], [[0, 3, 4], [1, 3, 4], [2, 4, 3]], (2, 2, 2),
        [0, 0, 0, 1, 2], [[0, 1, 2]],
        # s is clamped before the fraction is taken: 2.0 and 7.0 both count as the far face (r = 2^20), -3.0 as the near one (r = 0)
        out_v=[[(1.5 + 2.0 + 2.0) / 3, .5, .5], [0.0, 0.0, .5], [2.0, 2.0, 0.0]]),
}


def hand(name):
    return HAND[name]

"""The rules of include/crnerf_mesh_parts.h restated in NumPy, and the fields the mesh-parts tests run on (tests/test_mesh_parts_host.py,
tests/test_gpu_mesh_parts.py).  Test infrastructure: written from the rules, not from csrc/mesh_parts.hip -- the labels come from min-label
propagation over the faces with pointer jumping, where the kernel runs a union-find.

parts_ref(faces, V)   -> (vertex_part [V] int32, face_part [F] int32, part_vertices [K] int32, part_faces [K] int32)
select_ref(vertices, faces, normals, vertex_part, face_part, keep) -> (vertices', faces', normals')
largest_ref(part_faces, n) -> keep [K] uint8
The meshes are built with tests/_mesh_cases.py (mesh_ref) and kept, once per case, in MESHES."""
import numpy as np

import _mesh_cases as M


def valid_faces(faces, V):
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    return ((f >= 0) & (f < V)).all(axis=1)


def propagation_rounds(faces, V):
    """Rounds of NAIVE min-label propagation (no pointer jumping) until nothing changes: how far labels have to travel."""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    f = f[valid_faces(f, V)]
    label = np.arange(V, dtype=np.int64)
    rounds = 0
    while True:
        new = label.copy()
        np.minimum.at(new, f.reshape(-1), np.repeat(label[f].min(axis=1), 3))
        if np.array_equal(new, label):
            return rounds
        label, rounds = new, rounds + 1


def parts_ref(faces, V):
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    V = int(V)
    ok = valid_faces(f, V)
    fv = f[ok]
    label = np.arange(V, dtype=np.int64)
    if len(fv):
        flat = fv.reshape(-1)
        order = np.argsort(flat, kind="stable")                  # the corners grouped by vertex, once
        used, starts = np.unique(flat[order], return_index=True)
        while True:
            m = np.repeat(label[fv].min(axis=1), 3)              # every corner is offered the smallest label of its face
            new = label.copy()
            new[used] = np.minimum(label[used], np.minimum.reduceat(m[order], starts))
            while True:                                          # pointer jumping: label[v] <= v names a vertex of v's part
                hop = new[new]
                if np.array_equal(hop, new):
                    break
                new = hop
            if np.array_equal(new, label):
                break
            label = new
    roots = np.nonzero(label == np.arange(V))[0]                 # a part's label is its smallest vertex id: ascending roots = ascending ids
    part_of_root = np.full(V, -1, dtype=np.int64)
    part_of_root[roots] = np.arange(len(roots))
    vertex_part = part_of_root[label].astype(np.int32)
    face_part = np.full(len(f), -1, dtype=np.int32)
    face_part[ok] = vertex_part[fv[:, 0]]
    K = len(roots)
    return (vertex_part, face_part, np.bincount(vertex_part, minlength=K).astype(np.int32),
            np.bincount(face_part[ok], minlength=K).astype(np.int32))


def select_ref(vertices, faces, normals, vertex_part, face_part, keep):
    keep = np.asarray(keep).astype(bool)
    K = len(keep)
    vp, fp = np.asarray(vertex_part, dtype=np.int64), np.asarray(face_part, dtype=np.int64)
    kv = np.zeros(len(vp), dtype=bool)
    inside = (vp >= 0) & (vp < K)
    kv[inside] = keep[vp[inside]]
    kf = np.zeros(len(fp), dtype=bool)
    inside = (fp >= 0) & (fp < K)
    kf[inside] = keep[fp[inside]]
    new_id = np.cumsum(kv) - kv                                  # the rank among the kept
    out_f = new_id[np.asarray(faces, dtype=np.int64).reshape(-1, 3)[kf]].astype(np.int32).reshape(-1, 3)
    return np.asarray(vertices)[kv], out_f, None if normals is None else np.asarray(normals)[kv]


def largest_ref(part_faces, n):
    pf = np.asarray(part_faces, dtype=np.int64)
    order = sorted(range(len(pf)), key=lambda k: (-pf[k], k))    # size descending, ties to the smaller id
    keep = np.zeros(len(pf), dtype=np.uint8)
    keep[order[:n]] = 1
    return keep


# ---------------------------------------------------------------------------------------------------------------- hand cases
# name -> (faces, V, vertex_part, face_part): small enough to label by eye
HAND = {
    "empty": (np.zeros((0, 3), np.int32), 0, [], []),
    "no faces": (np.zeros((0, 3), np.int32), 5, [0, 1, 2, 3, 4], []),
    "one triangle": ([[0, 1, 2]], 3, [0, 0, 0], [0]),
    "two disjoint triangles": ([[0, 1, 2], [3, 4, 5]], 6, [0, 0, 0, 1, 1, 1], [0, 1]),
    "interleaved ids": ([[0, 2, 4], [1, 3, 5]], 6, [0, 1, 0, 1, 0, 1], [0, 1]),
    "one shared vertex": ([[0, 1, 2], [2, 3, 4]], 5, [0, 0, 0, 0, 0], [0, 0]),
    "duplicate face": ([[0, 1, 2], [0, 1, 2], [3, 4, 5]], 6, [0, 0, 0, 1, 1, 1], [0, 0, 1]),
    "unreferenced vertex in the middle": ([[0, 1, 2], [4, 5, 6]], 7, [0, 0, 0, 1, 2, 2, 2], [0, 2]),
    "bad ids": ([[0, 1, 2], [2, -1, 3], [3, 4, 5], [5, 6, 0], [4, 5, 3]], 6, [0, 0, 0, 1, 1, 1], [0, -1, 1, -1, 1]),
    "a chain joined from the far end": ([[6, 7, 8], [4, 5, 6], [2, 3, 4], [0, 1, 2]], 9, [0] * 9, [0, 0, 0, 0]),
    "degenerate face": ([[1, 1, 1], [0, 0, 2]], 4, [0, 1, 0, 2], [1, 0]),
}


def hand(name):
    faces, V, vp, fp = HAND[name]
    return np.asarray(faces, dtype=np.int32).reshape(-1, 3), V, np.asarray(vp, dtype=np.int32), np.asarray(fp, dtype=np.int32)


# ---------------------------------------------------------------------------------------------------------------- fields
BLOB_SPHERES = ((-.35, -.3, -.3, .45), (.6, .6, .6, .2), (.65, -.6, .1, .12), (-.7, .7, .6, .07), (.95, 0, -.7, .15))
BLOB_CAVITY = (-.35, -.3, -.3, .15)


def _grid(nx, ny=None, nz=None):
    ny, nz = ny or nx, nz or nx
    xs, ys, zs = (np.linspace(-1.0, 1.0, n, dtype=np.float32) for n in (nx, ny, nz))
    Z, Y, X = np.meshgrid(zs.astype(np.float64), ys.astype(np.float64), xs.astype(np.float64), indexing="ij")
    return (xs, ys, zs), (X, Y, Z)


def blobs(n):
    """(sigma, xs, ys, zs), threshold 0: five spheres, the first cut by the box and hollowed by a cavity."""
    axes, (X, Y, Z) = _grid(n)
    s = np.full(X.shape, -np.inf)
    for cx, cy, cz, r in BLOB_SPHERES:
        s = np.maximum(s, r * r - ((X - cx) ** 2 + (Y - cy) ** 2 + (Z - cz) ** 2))
    cx, cy, cz, r = BLOB_CAVITY
    s = np.minimum(s, -(r * r - ((X - cx) ** 2 + (Y - cy) ** 2 + (Z - cz) ** 2)))
    return (s.astype(np.float32),) + axes


def tie():
    """Two spheres that are exact translates of one another (integer index arithmetic) on a 33^3 grid: equal face counts."""
    axes, _ = _grid(33)
    iz, iy, ix = np.meshgrid(np.arange(33), np.arange(33), np.arange(33), indexing="ij")
    s = np.full(ix.shape, -np.inf)
    for cx, cy, cz in ((8, 9, 10), (22, 21, 20)):
        s = np.maximum(s, 30.5 - ((ix - cx) ** 2 + (iy - cy) ** 2 + (iz - cz) ** 2))
    return (s.astype(np.float32),) + axes


def helix():
    """A helical tube on 65 x 65 x 49: radius 0.7, 5 turns, z from -0.8 to 0.8, tube radius 0.09 -- one long part."""
    axes, (X, Y, Z) = _grid(65, 65, 49)
    phi = np.mod(np.arctan2(Y, X), 2 * np.pi)
    d2 = np.full(X.shape, np.inf)
    for k in range(-1, 7):                                       # the centre-line point at the node's own angle, on every turn; clamped to the ends
        t = np.clip((phi + 2 * np.pi * k) / (10 * np.pi), 0.0, 1.0)
        d2 = np.minimum(d2, (X - 0.7 * np.cos(10 * np.pi * t)) ** 2 + (Y - 0.7 * np.sin(10 * np.pi * t)) ** 2 + (Z - (-0.8 + 1.6 * t)) ** 2)
    return ((0.09 ** 2 - d2).astype(np.float32),) + axes


def noise(n, offset):
    """Uniform noise in [-1, 1] from default_rng(5) at n^3, plus an offset."""
    axes, _ = _grid(n)
    s = np.random.default_rng(5).uniform(-1.0, 1.0, (n, n, n)) + offset
    return (s.astype(np.float32),) + axes


FIELDS = {
    "blobs33": lambda: blobs(33), "blobs17": lambda: blobs(17), "tie": tie, "helix": helix,
    "noise41-0.75": lambda: noise(41, -0.75), "noise41-0.6": lambda: noise(41, -0.6), "noise73+0.35": lambda: noise(73, 0.35),
}
MESHES, PARTS = {}, {}


def mesh(name):
    """(vertices float32, faces int32, normals float32) of the named field at threshold 0, by the restatement of crnerf_mesh.h; computed once."""
    if name not in MESHES:
        v, f, n = M.mesh_ref(*FIELDS[name](), 0.0)
        for a in (v, f):
            a.setflags(write=False)
        n = n.astype(np.float32)
        n.setflags(write=False)
        MESHES[name] = (v, f, n)
    return MESHES[name]


def parts(name):
    """parts_ref of mesh(name); computed once."""
    if name not in PARTS:
        v, f, _ = mesh(name)
        PARTS[name] = parts_ref(f, len(v))
        for a in PARTS[name]:
            a.setflags(write=False)
    return PARTS[name]

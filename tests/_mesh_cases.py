"""The rules of include/crnerf_mesh.h restated in vectorised NumPy, the fields the mesh tests run on, and the topology bookkeeping they share
(tests/test_mesh_host.py, tests/test_gpu_mesh.py).  Test infrastructure: written from the rules, not from csrc/mesh.hip -- the orientation of every
(tet, pattern) case is found here geometrically, in float64 on the unit cube, where the kernel derives an integer table at compile time.

mesh_ref(sigma, xs, ys, zs, threshold) -> (vertices [V,3] float32, faces [F,3] int32, normals [V,3] float64):
  vertices with the two-rounding float32 interpolation (NumPy rounds every float32 operation on its own), normals in float64 from the float32 grid
  with the float32 t of the vertex."""
import itertools

import numpy as np

PERMS = list(itertools.permutations(range(3)))          # xyz, xzy, yxz, yzx, zxy, zyx: tet 0..5
assert PERMS == [(0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)]


def _tet_nodes(perm):
    """The four nodes of a tet as offsets (dx, dy, dz) from the cell's origin: the monotone path along the axes of perm."""
    n, path = [0, 0, 0], [(0, 0, 0)]
    for a in perm:
        n[a] += 1
        path.append(tuple(n))
    return path


def _case_cycle(perm, pattern):
    """The oriented cycle of a (tet, inside pattern) case: a list of (node j, node k) path indices, j < k, one per active edge; [] when the pattern
    has no sign change.  Bit j of pattern: path node j is inside."""
    nodes = np.array(_tet_nodes(perm), dtype=np.float64)
    I = [j for j in range(4) if (pattern >> j) & 1]
    O = [j for j in range(4) if not (pattern >> j) & 1]
    if not I or not O:
        return []
    if len(I) == 1:
        cyc = [(I[0], o) for o in O]
    elif len(O) == 1:
        cyc = [(i, O[0]) for i in I]
    else:
        cyc = [(I[0], O[0]), (I[0], O[1]), (I[1], O[1]), (I[1], O[0])]
    p = [0.5 * (nodes[a] + nodes[b]) for a, b in cyc]           # any 0 < t < 1 gives the same sense; the midpoints will do
    nrm = np.cross(p[1] - p[0], p[2] - p[0])
    if len(p) == 4:
        nrm = nrm + np.cross(p[2] - p[0], p[3] - p[0])
    out = nodes[O].mean(0) - nodes[I].mean(0)
    s = float(np.dot(nrm, out))
    assert abs(s) > 1e-9
    if s < 0:
        cyc = cyc[::-1]
    return [(min(a, b), max(a, b)) for a, b in cyc]


def _node_gradient(s64, axes64):
    """[3, nz, ny, nx]: d sigma / d (x, y, z) at the nodes -- central differences, one-sided at the border, over the actual spacing."""
    out = []
    for axis, ax in ((2, axes64[0]), (1, axes64[1]), (0, axes64[2])):
        n = s64.shape[axis]
        hi, lo = np.minimum(np.arange(n) + 1, n - 1), np.maximum(np.arange(n) - 1, 0)
        shape = [1, 1, 1]
        shape[axis] = n
        with np.errstate(all="ignore"):
            out.append((np.take(s64, hi, axis=axis) - np.take(s64, lo, axis=axis)) / (ax[hi] - ax[lo]).reshape(shape))
    return np.stack(out)


def mesh_ref(sigma, xs, ys, zs, threshold, want_normals=True):
    s = np.asarray(sigma, dtype=np.float32)
    xs, ys, zs = (np.asarray(a, dtype=np.float32) for a in (xs, ys, zs))
    nz, ny, nx = s.shape
    assert (nz, ny, nx) == (len(zs), len(ys), len(xs))
    empty = (np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32), np.zeros((0, 3), np.float64))
    if min(nx, ny, nz) < 2:
        return empty
    thr = np.float32(threshold)
    with np.errstate(invalid="ignore"):
        inside = s > thr
    # ---- active edges, vertex ids in (node, direction) order
    active = np.zeros((nz, ny, nx, 7), dtype=bool)
    for d in range(7):
        dx, dy, dz = (d + 1) & 1, ((d + 1) >> 1) & 1, (d + 1) >> 2
        active[:nz - dz, :ny - dy, :nx - dx, d] = inside[:nz - dz, :ny - dy, :nx - dx] != inside[dz:, dy:, dx:]
    vid = (np.cumsum(active.reshape(-1), dtype=np.int64) - 1).reshape(active.shape)
    vid[~active] = -1
    node, d = np.nonzero(active.reshape(-1, 7))                  # row-major: node ascending, then direction
    ix, iy, iz = node % nx, (node // nx) % ny, node // (nx * ny)
    jx, jy, jz = ix + ((d + 1) & 1), iy + (((d + 1) >> 1) & 1), iz + ((d + 1) >> 2)
    sa, sb = s[iz, iy, ix], s[jz, jy, jx]
    with np.errstate(all="ignore"):
        t = (thr - sa) / (sb - sa)                               # float32 throughout
        t = np.where(np.isfinite(t) & (t >= 0) & (t <= 1), t, np.float32(0.5)).astype(np.float32)
        verts = np.stack([a[i] + t * (a[j] - a[i]) for a, i, j in ((xs, ix, jx), (ys, iy, jy), (zs, iz, jz))], axis=1).astype(np.float32)
    # ---- faces
    cz, cy, cx = np.meshgrid(np.arange(nz - 1), np.arange(ny - 1), np.arange(nx - 1), indexing="ij")
    cz, cy, cx = cz.reshape(-1), cy.reshape(-1), cx.reshape(-1)
    cell_flat = cx + nx * (cy + ny * cz)
    keys, tris = [], []                                          # keys: (cell, tet, triangle within the tet)
    for tet, perm in enumerate(PERMS):
        nodes = _tet_nodes(perm)
        ins = [inside[cz + o[2], cy + o[1], cx + o[0]] for o in nodes]
        pattern = sum(b.astype(np.int64) << j for j, b in enumerate(ins))
        for pat in range(1, 15):
            sel = np.nonzero(pattern == pat)[0]
            if sel.size == 0:
                continue
            ids = []
            for a, b in _case_cycle(perm, pat):
                oa, ob = nodes[a], nodes[b]
                dirn = (ob[0] - oa[0]) + 2 * (ob[1] - oa[1]) + 4 * (ob[2] - oa[2]) - 1
                v = vid[cz[sel] + oa[2], cy[sel] + oa[1], cx[sel] + oa[0], dirn]
                assert (v >= 0).all()
                ids.append(v)
            poly = np.stack(ids, axis=1)
            n = poly.shape[1]
            rot = (np.argmin(poly, axis=1)[:, None] + np.arange(n)[None, :]) % n
            poly = np.take_along_axis(poly, rot, axis=1)
            for k, tri in enumerate([(0, 1, 2)] if n == 3 else [(0, 1, 2), (0, 2, 3)]):
                keys.append(np.stack([cell_flat[sel], np.full(sel.size, tet), np.full(sel.size, k)], axis=1))
                tris.append(poly[:, tri])
    if not tris:
        faces = np.zeros((0, 3), np.int32)
    else:
        keys, tris = np.concatenate(keys), np.concatenate(tris)
        order = np.lexsort((keys[:, 2], keys[:, 1], keys[:, 0]))
        faces = tris[order].astype(np.int32)
    if not want_normals:
        return verts, faces, None
    # ---- normals, float64
    g = _node_gradient(s.astype(np.float64), [a.astype(np.float64) for a in (xs, ys, zs)])
    with np.errstate(all="ignore"):
        ga, gb = g[:, iz, iy, ix].T, g[:, jz, jy, jx].T
        gi = ga + t.astype(np.float64)[:, None] * (gb - ga)
        ln = np.linalg.norm(gi, axis=1)
        nrm = np.where((ln > 0)[:, None], -gi / ln[:, None], 0.0)
    return verts, faces, nrm


def interpolated_gradient_norm(sigma, xs, ys, zs, threshold):
    """Per vertex of mesh_ref: |gradient interpolated along the edge| in float64; and the largest node gradient norm of the field."""
    s = np.asarray(sigma, dtype=np.float32)
    nz, ny, nx = s.shape
    g = _node_gradient(s.astype(np.float64), [np.asarray(a, np.float64) for a in (xs, ys, zs)])
    inside = s > np.float32(threshold)
    active = np.zeros((nz, ny, nx, 7), dtype=bool)
    for d in range(7):
        dx, dy, dz = (d + 1) & 1, ((d + 1) >> 1) & 1, (d + 1) >> 2
        active[:nz - dz, :ny - dy, :nx - dx, d] = inside[:nz - dz, :ny - dy, :nx - dx] != inside[dz:, dy:, dx:]
    node, d = np.nonzero(active.reshape(-1, 7))
    ix, iy, iz = node % nx, (node // nx) % ny, node // (nx * ny)
    jx, jy, jz = ix + ((d + 1) & 1), iy + (((d + 1) >> 1) & 1), iz + ((d + 1) >> 2)
    thr = np.float32(threshold)
    t = ((thr - s[iz, iy, ix]) / (s[jz, jy, jx] - s[iz, iy, ix])).astype(np.float64)
    ga, gb = g[:, iz, iy, ix].T, g[:, jz, jy, jx].T
    return np.linalg.norm(ga + t[:, None] * (gb - ga), axis=1), float(np.linalg.norm(g, axis=0).max())


# ---------------------------------------------------------------------------------------------------------------- topology
def topology(faces, n_vertices):
    """Edge bookkeeping of an indexed triangle list: uses of every undirected edge, the largest use count of a directed edge, E, the Euler
    characteristic V - E + F, the number of unreferenced vertices, and the undirected edges used once (as [k,2] vertex ids)."""
    f = np.asarray(faces, dtype=np.int64)
    a = np.concatenate([f[:, 0], f[:, 1], f[:, 2]])
    b = np.concatenate([f[:, 1], f[:, 2], f[:, 0]])
    V = int(n_vertices)
    _, dcount = np.unique(a * V + b, return_counts=True)
    ukey, ucount = np.unique(np.minimum(a, b) * V + np.maximum(a, b), return_counts=True)
    once = ukey[ucount == 1]
    return {"uses": {int(k): int(v) for k, v in zip(*np.unique(ucount, return_counts=True))},
            "directed_max": int(dcount.max()) if dcount.size else 0,
            "E": int(ukey.size), "chi": V - int(ukey.size) + int(f.shape[0]),
            "unused": V - int(np.unique(f).size), "once": np.stack([once // V, once % V], axis=1) if V else np.zeros((0, 2), np.int64)}


def face_normals(vertices, faces):
    v = np.asarray(vertices, dtype=np.float64)
    f = np.asarray(faces, dtype=np.int64)
    return np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])


def signed_volume(vertices, faces):
    v = np.asarray(vertices, dtype=np.float64)
    f = np.asarray(faces, dtype=np.int64)
    return float(np.einsum("ij,ij->i", v[f[:, 0]], np.cross(v[f[:, 1]], v[f[:, 2]])).sum() / 6.0)


# ---------------------------------------------------------------------------------------------------------------- fields
SPHERE_R, TORUS_R, TORUS_r = 0.7, 0.6, 0.25


def _lin(n):
    ax = np.linspace(-1.0, 1.0, n, dtype=np.float32)
    return ax, np.meshgrid(ax, ax, ax, indexing="ij")           # Z, Y, X


def sphere(n):
    """(sigma, xs, ys, zs), threshold 0: R^2 - |p|^2 on linspace(-1, 1, n) axes."""
    ax, (Z, Y, X) = _lin(n)
    return (SPHERE_R * SPHERE_R - (X * X + Y * Y + Z * Z)).astype(np.float32), ax, ax, ax


def torus(n):
    ax, (Z, Y, X) = _lin(n)
    return (TORUS_r ** 2 - ((np.sqrt(X * X + Y * Y) - TORUS_R) ** 2 + Z * Z)).astype(np.float32), ax, ax, ax


def plane(n):
    """A tilted plane through the box: an open surface whose border lies on the box's faces."""
    ax, (Z, Y, X) = _lin(n)
    return (0.13 - Z + 0.3 * X + 0.11 * Y).astype(np.float32), ax, ax, ax


def uneven_axes(shape, rng):
    """Strictly increasing, non-uniform, different per axis: cumulated spacings in [0.5, 1.5] scaled to a few units."""
    out = []
    for n, (lo, span) in zip(shape, ((-1.5, 3.0), (-1.0, 2.5), (0.25, 2.0))):
        steps = np.concatenate([[0.0], np.cumsum(rng.uniform(0.5, 1.5, max(n - 1, 0)))])
        out.append((lo + span * steps / max(steps[-1], 1.0)).astype(np.float32))
    return out


def smooth_field(shape):
    """(sigma, xs, ys, zs) for shape = (nx, ny, nz), threshold 0: a few low-frequency waves with seeded phases on uneven axes; the seed is the
    shape.  Both signs occur, and no node sits on the threshold."""
    rng = np.random.default_rng([21] + list(shape))
    xs, ys, zs = uneven_axes(shape, rng)
    Z, Y, X = np.meshgrid(zs.astype(np.float64), ys.astype(np.float64), xs.astype(np.float64), indexing="ij")
    s = np.zeros_like(X)
    for _ in range(5):
        k = rng.uniform(-2.5, 2.5, 3)
        s += rng.uniform(0.4, 1.0) * np.sin(k[0] * X + k[1] * Y + k[2] * Z + rng.uniform(0, 2 * np.pi))
    s = s.astype(np.float32)
    assert (s > 0).any() and (s < 0).any() and not (s == 0).any()
    return s, xs, ys, zs


ONE_CELL_THRESHOLD = 0.1
ONE_CELL_AXES = (np.array([-0.3, 0.9], np.float32), np.array([0.1, 0.45], np.float32), np.array([-1.2, -0.2], np.float32))


def one_cell(pattern):
    """The 2 x 2 x 2 grid whose corner k = dx + 2 dy + 4 dz is inside iff bit k of pattern is set: threshold +- a seeded magnitude in [0.2, 1]."""
    mag = np.random.default_rng(1000 + pattern).uniform(0.2, 1.0, 8)
    s = np.empty((2, 2, 2), np.float32)
    for k in range(8):
        s[k >> 2, (k >> 1) & 1, k & 1] = ONE_CELL_THRESHOLD + (mag[k] if (pattern >> k) & 1 else -mag[k])
    return s

"""GPU checks of the mesh extraction (include/crnerf_mesh.h, ops.mesh_grid, crnerf_amd.geometry): marching tetrahedra on the Kuhn split, on the device.

  1. One cell, all 256 inside patterns, against the NumPy restatement (tests/_mesh_cases.py) bit for bit: the case table and its orientation.
  2. Shared vertices and index arithmetic: larger grids against the restatement, faces and vertices bit for bit, normals to 4e-6.
  3. Topology without the restatement: sphere and torus at 65^3 are closed, oriented, of the right genus, and where they should be.
  4. An open surface ends on the box.   5. Edge values: threshold-valued, NaN, +inf, overflowing nodes; empty results.
  6. Determinism and plumbing: equal bytes, normals=False, capacities, extract_mesh, PLY.
"""
import ctypes
import math

import numpy as np
import pytest
import torch

from crnerf_amd import _lib, geometry, ops
from crnerf_amd.models.nerf import NeRF_sigma

import _geometry_cases as G
import _mesh_cases as M

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def dev(*arrays):
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in arrays)


def run(field, threshold, normals=True):
    v, f, n = ops.mesh_grid(*dev(*field), threshold, normals=normals)
    assert v.dtype == torch.float32 and f.dtype == torch.int32 and v.dim() == 2 and v.shape[1] == 3 and f.dim() == 2 and f.shape[1] == 3
    assert v.is_contiguous() and f.is_contiguous() and v.device == f.device == torch.device(DEV)
    assert (n is None) == (not normals) and (n is None or (n.dtype == torch.float32 and n.shape == v.shape))
    return v.cpu().numpy(), f.cpu().numpy(), None if n is None else n.cpu().numpy()


def assert_same_mesh(got, want, what):
    """Faces and vertices bit for bit (torch.equal compares values: the bits, NaN and -0 aside, and neither occurs)."""
    (v, f, _), (rv, rf, _) = got, want
    assert v.shape == rv.shape and f.shape == rf.shape, (what, v.shape, rv.shape, f.shape, rf.shape)
    assert torch.equal(torch.from_numpy(f), torch.from_numpy(rf)), what
    assert torch.equal(torch.from_numpy(v), torch.from_numpy(rv)), what
    assert np.array_equal(v.view(np.uint32), rv.view(np.uint32)), what


# ---------------------------------------------------------------- 1. one cell, exhaustively
def test_one_cell_all_256_patterns():
    n_faces = 0
    for pattern in range(256):
        field = (M.one_cell(pattern),) + M.ONE_CELL_AXES
        got, want = run(field, M.ONE_CELL_THRESHOLD), M.mesh_ref(*field, M.ONE_CELL_THRESHOLD)
        assert_same_mesh(got, want, "pattern %d" % pattern)
        n_faces += len(got[1])
        if pattern in (0, 255):
            assert len(got[0]) == 0 and len(got[1]) == 0
        else:
            assert len(got[1]) >= 2           # every corner lies in at least two of the six tetrahedra
            # orientation, without the restatement, where one corner is the odd one: the faces form a fan around it and all look away from an
            # inside corner, or all at an outside one
            inside = field[0] > np.float32(M.ONE_CELL_THRESHOLD)
            if inside.sum() in (1, 7):
                iz, iy, ix = np.argwhere(inside if inside.sum() == 1 else ~inside)[0]
                odd = np.array([field[1][ix], field[2][iy], field[3][iz]], np.float64)
                fn, cen = M.face_normals(got[0], got[1]), got[0][got[1]].astype(np.float64).mean(1)
                d = np.einsum("ij,ij->i", fn, cen - odd)
                assert (d > 0).all() if inside.sum() == 1 else (d < 0).all(), pattern
    assert n_faces > 0


# ---------------------------------------------------------------- 2. shared vertices and index arithmetic
# (nx, ny, nz).  Both passes walk the FLAT node index: the count pass scans 1,024 consecutive nodes per workgroup, four per thread, and the emit pass
# takes 4,096 per workgroup, sixteen per thread.  (70, 33, 17) = 39,270 nodes is 39 scan blocks and 10 emit blocks whose seams -- and the threads'
# runs of 4 and 16 -- fall inside rows, across row ends and across slab ends alike, and it ends on a partial run of either kind (39,270 = 4 k + 2 =
# 16 k + 6); there is no tile in x, y or z to cross.  The ONE boundary it does not reach is the chunk of the block-total scan (1,024 block totals =
# 1,048,576 nodes a chunk): (129, 97, 85) = 1,063,605 nodes is the smallest shape of this kind (odd, distinct axes) past it, 1,039 block totals in
# two chunks.
SHAPES = [(3, 3, 3), (5, 4, 3), (2, 7, 2), (70, 33, 17), (129, 97, 85)]
# about a dozen fp32 roundings of 2^-24 each before a normalisation that does not amplify: below 1e-6; the bar is four times that
NORMAL_BAR = 4e-6


@pytest.mark.parametrize("shape", SHAPES)
def test_grids_against_the_restatement(shape):
    field = M.smooth_field(shape)
    got, want = run(field, 0.0), M.mesh_ref(*field, 0.0)
    assert len(want[0]) > 0 and len(want[1]) > 0
    assert_same_mesh(got, want, shape)
    gnorm, gmax = M.interpolated_gradient_norm(*field, 0.0)
    keep = gnorm >= 1e-3 * gmax
    assert keep.sum() >= 0.9 * len(keep)
    err = float(np.abs(got[2].astype(np.float64) - want[2])[keep].max())
    print("normals, shape %s: V %d F %d, max |d| %.3e over %d of %d vertices" % (shape, len(got[0]), len(got[1]), err, keep.sum(), len(keep)))
    assert err <= NORMAL_BAR
    length = np.linalg.norm(got[2].astype(np.float64), axis=1)
    assert np.abs(length[keep] - 1).max() < 1e-6


# ---------------------------------------------------------------- 3. topology, without the restatement
_CLOSED = {}


def closed(name):
    if name not in _CLOSED:
        _CLOSED[name] = run({"sphere": M.sphere, "torus": M.torus}[name](65), 0.0)
    return _CLOSED[name]


@pytest.mark.parametrize("name,chi", [("sphere", 2), ("torus", 0)])
def test_closed_surfaces_are_closed_oriented_and_of_the_right_genus(name, chi):
    v, f, _ = closed(name)
    t = M.topology(f, len(v))
    assert t["uses"] == {2: t["E"]}          # every undirected edge in exactly two faces
    assert t["directed_max"] == 1            # every directed edge in at most one: the two faces at an edge agree on the orientation
    assert t["chi"] == chi
    assert t["unused"] == 0 and f.min() == 0 and f.max() == len(v) - 1


def test_the_sphere_is_where_it_should_be():
    v, f, n = closed("sphere")
    R, h = M.SPHERE_R, 2.0 / 64
    centres = v[f].astype(np.float64).mean(1)
    assert (np.einsum("ij,ij->i", M.face_normals(v, f), centres) > 0).all()      # every face normal points away from the centre
    r = np.linalg.norm(v.astype(np.float64), axis=1)
    print("sphere 65^3: V %d F %d, radius in [R - %.3e, R + %.3e]; 3 h^2 / (8 R) = %.3e" % (len(v), len(f), R - r.min(), r.max() - R, 3 * h * h / (8 * R)))
    # linear interpolation of a quadratic field along an edge of at most sqrt(3) h puts the vertex inside by at most 3 h^2 / (8 R) to leading order;
    # the bar is 4/3 of that
    assert r.min() >= R - h * h / (2 * R) and r.max() <= R + 1e-6
    ratio = M.signed_volume(v, f) / (4.0 * math.pi * R ** 3 / 3.0)
    print("sphere 65^3: volume / (4 pi R^3 / 3) = 1 - %.3f h^2 / R^2" % ((1 - ratio) / (h * h / (R * R))))
    assert 1 - h * h / (R * R) <= ratio <= 1
    unit = v.astype(np.float64) / r[:, None]
    assert np.einsum("ij,ij->i", n.astype(np.float64), unit).min() > 0.999         # the vertex normals: outward as well


# ---------------------------------------------------------------- 4. an open surface
def test_an_open_surface_ends_on_the_box():
    field = M.plane(33)
    v, f, _ = run(field, 0.0)
    t = M.topology(f, len(v))
    assert set(t["uses"]) == {1, 2} and t["directed_max"] == 1 and t["unused"] == 0
    on_box = (np.abs(v) == 1.0).any(axis=1)            # the axes end at exactly -1 and 1, and a coordinate an edge does not move along is copied
    once = t["once"]
    assert len(once) > 0 and on_box[once[:, 0]].all() and on_box[once[:, 1]].all()
    assert t["chi"] == 1                                # a disc


# ---------------------------------------------------------------- 5. edge values
def test_a_node_on_the_threshold_is_outside_and_its_degenerate_triangles_stay():
    s = -np.ones((5, 5, 5), np.float32)
    s[2, 2, 2] = 1.0                 # A, inside
    s[2, 1, 2] = 1.0                 # B, inside
    s[2, 2, 3] = 0.0                 # T = (ix 3, iy 2, iz 2): ON the threshold, joined to A along x and to B along the xy diagonal
    ax = np.array([-1.0, -0.5, 0.25, 0.5, 1.0], np.float32)
    field = (s, ax, ax, ax)
    got = run(field, 0.0)
    assert_same_mesh(got, M.mesh_ref(*field, 0.0), "threshold node")
    v, f, _ = got
    at_T = (v == np.array([0.5, 0.25, 0.25], np.float32)).all(axis=1)
    assert at_T.sum() == 2           # T is outside: both edges to the inside nodes are active, and t puts their vertices ON T
    t = M.topology(f, len(v))
    assert t["uses"] == {2: t["E"]} and t["chi"] == 2 and t["unused"] == 0      # the topology is what is promised
    area = np.linalg.norm(M.face_normals(v, f), axis=1)
    both = at_T[f].sum(axis=1) == 2
    assert both.any() and (area[both] == 0).all() and (area[~both] > 0).all()


def test_nan_inf_and_overflow_fall_back_to_the_midpoint():
    field = list(M.smooth_field((6, 5, 4)))
    s = field[0] = field[0].copy()
    s[:] = -np.abs(s) - 0.1                       # everything outside ...
    s[1, 1, 1] = np.nan                           # ... a NaN node: outside, no vertex around it
    s[2, 3, 4] = np.inf                           # a +inf node: inside; it owns edges (thr - inf) / (sb - inf) = NaN -> 0.5, the others get t = 0 or 1
    s[1, 3, 2], s[1, 3, 3] = 3e38, -3e38          # sb - sa overflows
    s[2, 1, 1] = 1.0                              # a finite inside node next to the NaN: t = NaN on that edge
    got = run(field, 0.0)
    want = M.mesh_ref(*field, 0.0)
    assert_same_mesh(got, want, "non-finite nodes")
    v, f, n = got
    assert np.isfinite(v).all() and len(v) > 0 and len(f) > 0
    xs, ys, zs = field[1:]
    mid = lambda a, i: np.float32(a[i] + np.float32(0.5) * (a[i + 1] - a[i]))      # noqa: E731
    # the edge from the NaN node (1,1,1) up to (1,1,2) = the inside node s[2,1,1]: the midpoint in z, x and y copied
    assert (v == np.array([xs[1], ys[1], mid(zs, 1)], np.float32)).all(axis=1).sum() == 1
    # the +inf node (ix 4, iy 3, iz 2) owns the edge to (5,3,2): the midpoint in x
    assert (v == np.array([mid(xs, 4), ys[3], zs[2]], np.float32)).all(axis=1).sum() == 1
    t = M.topology(f, len(v))
    assert t["unused"] == 0 and t["directed_max"] == 1


def test_nothing_to_extract():
    field = M.smooth_field((9, 8, 7))
    lo, hi = float(field[0].min()), float(field[0].max())
    for thr in (hi, hi + 1.0, np.nextafter(np.float32(lo), np.float32(-np.inf)), lo - 1.0, float("inf"), float("-inf")):
        v, f, n = run(field, float(thr))
        assert v.shape == (0, 3) and f.shape == (0, 3) and n.shape == (0, 3), thr
    assert len(run(field, lo)[0]) > 0              # strictly above: the minimum itself is outside, everything else inside
    s, xs, ys, zs = field
    for cut in ((slice(None), slice(None), slice(0, 1)), (slice(None), slice(0, 1), slice(None)), (slice(0, 1), slice(None), slice(None))):
        short = (s[cut], xs[cut[2]], ys[cut[1]], zs[cut[0]])
        v, f, n = run(short, 0.0)
        assert v.shape == (0, 3) and f.shape == (0, 3) and n.shape == (0, 3)
    v, f, n = ops.mesh_grid(torch.zeros(0, 4, 4, device=DEV), torch.zeros(4, device=DEV), torch.zeros(4, device=DEV), torch.zeros(0, device=DEV), 0.0)
    assert v.shape == (0, 3) and f.shape == (0, 3)


# ---------------------------------------------------------------- 6. determinism and plumbing
def test_two_calls_give_equal_bytes_and_normals_are_optional():
    field = M.smooth_field((70, 33, 17))
    a, b, c = run(field, 0.0), run(field, 0.0), run(field, 0.0, normals=False)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()
    assert c[2] is None and c[0].tobytes() == a[0].tobytes() and c[1].tobytes() == a[1].tobytes()


def test_emit_stops_at_the_capacities():
    field = M.smooth_field((70, 33, 17))
    full = run(field, 0.0)
    sigma, xs, ys, zs = dev(*field)
    lib = _lib.load()
    dims = (70, 33, 17)
    ws = torch.empty(lib.crnerf_mesh_workspace_bytes(*dims), dtype=torch.uint8, device=DEV)
    counts = torch.full((2,), -1, dtype=torch.int64, device=DEV)
    p = lambda t: ctypes.c_void_p(t.data_ptr())      # noqa: E731
    _lib.check(lib.crnerf_mesh_count_f32(p(sigma), *dims, 0.0, p(ws), p(counts), _lib.stream_ptr()), "count")
    V, F = counts.tolist()
    assert (V, F) == (len(full[0]), len(full[1]))
    # V and F rows each, the last one a guard: emit is told of V - 1 and F - 1
    v = torch.full((V, 3), -7.0, device=DEV)
    n = torch.full((V, 3), -7.0, device=DEV)
    f = torch.full((F, 3), -7, dtype=torch.int32, device=DEV)
    _lib.check(lib.crnerf_mesh_emit_f32(p(sigma), p(xs), p(ys), p(zs), *dims, 0.0, p(ws), V - 1, F - 1, p(v), p(n), p(f), _lib.stream_ptr()), "emit")
    assert (v[V - 1] == -7.0).all() and (n[V - 1] == -7.0).all() and (f[F - 1] == -7).all()
    assert np.array_equal(v[:V - 1].cpu().numpy(), full[0][:V - 1]) and np.array_equal(n[:V - 1].cpu().numpy(), full[2][:V - 1])
    assert np.array_equal(f[:F - 1].cpu().numpy(), full[1][:F - 1])
    # far too short: the first rows, nothing else
    v.fill_(-7.0), f.fill_(-7)
    _lib.check(lib.crnerf_mesh_emit_f32(p(sigma), p(xs), p(ys), p(zs), *dims, 0.0, p(ws), 5, 3, p(v), None, p(f), _lib.stream_ptr()), "emit")
    assert (v[5:] == -7.0).all() and (f[3:] == -7).all()
    assert np.array_equal(v[:5].cpu().numpy(), full[0][:5]) and np.array_equal(f[:3].cpu().numpy(), full[1][:3])


class _Args:
    nerf_out_dim, img_wh = 64, [8, 8]


def test_extract_mesh_is_the_grid_then_the_mesh_and_ply_round_trip(tmp_path):
    m = NeRF_sigma("coarse", _Args(), in_channels_xyz=93, in_channels_dir=27).to(G.DEV)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in G.STATES[22].items()})
    m.eval()
    lo, hi, res = (-1.0, -0.5, 0.25), (1.0, 1.5, 2.0), (11, 6, 9)
    dg = geometry.density_grid(m, lo, hi, res)
    thr = float(dg.sigma.median())
    a, b = geometry.extract_mesh(m, lo, hi, res, thr), dg.mesh(thr)
    assert isinstance(a, geometry.Mesh) and a.vertices.shape[0] > 0 and a.faces.shape[0] > 0
    for name in ("vertices", "faces", "normals"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    v, f, n = ops.mesh_grid(dg.sigma, dg.xs, dg.ys, dg.zs, thr)
    assert torch.equal(a.vertices, v) and torch.equal(a.faces, f) and torch.equal(a.normals, n)
    assert dg.mesh(thr, normals=False).normals is None
    # PLY from device tensors
    path = str(tmp_path / "mesh.ply")
    a.save_ply(path)
    with open(path, "rb") as fh:
        blob = fh.read()
    end = blob.index(b"end_header\n") + 11
    V, F = a.vertices.shape[0], a.faces.shape[0]
    assert b"element vertex %d\n" % V in blob[:end] and b"element face %d\n" % F in blob[:end] and b"property float nz\n" in blob[:end]
    rows = np.frombuffer(blob, dtype="<f4", count=6 * V, offset=end).reshape(V, 6)
    tri = np.frombuffer(blob, dtype=np.dtype([("n", "u1"), ("i", "<i4", (3,))]), count=F, offset=end + 24 * V)
    assert end + 24 * V + 13 * F == len(blob) and (tri["n"] == 3).all()
    assert np.array_equal(rows[:, :3], a.vertices.cpu().numpy()) and np.array_equal(rows[:, 3:], a.normals.cpu().numpy())
    assert np.array_equal(tri["i"], a.faces.cpu().numpy())

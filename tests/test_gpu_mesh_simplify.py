"""GPU checks of the mesh simplification (csrc/crnerf_mesh_simplify.h, ops.mesh_cluster, crnerf_amd.geometry.Mesh.simplify,
extract_mesh(simplify_cell=)): vertex clustering on the device.  Vertices, faces, colours and vertex_cluster are compared bit for bit with the
NumPy restatement (tests/_mesh_simplify_cases.py); normals to within 2^-23 absolute per component -- one float32 ulp at 1: the only inexact steps
are a float64 sqrt, a float64 division and the final rounding.  Wherever a property of the simplified mesh is asserted it is asserted on the
restatement's output first, so a failure of the case itself shows up on the CPU.  The meshes are those of tests/_mesh_parts_cases.py.

  1. Hand cases.   2. blobs(33) at 2 and 4 grid spacings, with and without normals and colours.   3. Hot clusters: 148,181 vertices in 8 cells.
  4. Duplicate pressure: 200,000 faces over 64 clusters, both orientations, shuffled.   5. Past the chunk of the block-total scan and a table of
  2^23 slots: 1,164,962 vertices, 2,391,620 faces.   6. Determinism.   7. Plumbing: capacities, NULL normals / colours, parts / PLY, extract_mesh.
"""
import ctypes

import numpy as np
import pytest
import torch

from crnerf_amd import _lib, geometry, ops
from crnerf_amd.models.nerf import NeRF_sigma

import _geometry_cases as G
import _mesh_parts_cases as C
import _mesh_simplify_cases as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NORMAL_TOL = 2.0 ** -23


def dev(a):
    return torch.from_numpy(np.array(a, copy=True, order="C")).to(DEV)      # (a copy: the shared references are read-only)


def same(got, want, what):
    """Equal shape, dtype and bytes; got: a device tensor or None."""
    if want is None:
        assert got is None, what
        return
    g = got.cpu().numpy()
    assert g.dtype == want.dtype and g.shape == want.shape, (what, g.dtype, want.dtype, g.shape, want.shape)
    assert g.tobytes() == np.ascontiguousarray(want).tobytes(), what


def close_normals(got, want, what):
    if want is None:
        assert got is None, what
        return
    g = got.cpu().numpy()
    assert g.dtype == np.float32 and g.shape == want.shape, (what, g.dtype, g.shape, want.shape)
    worst = float(np.abs(g.astype(np.float64) - want.astype(np.float64)).max()) if g.size else 0.0
    print("%s: normals differ by at most %.3g (bound %.3g)" % (what, worst, NORMAL_TOL))
    assert worst <= NORMAL_TOL, (what, worst)


def same_cluster(got, want, what):
    """(vertices, faces, normals, colors, vertex_cluster) of ops.mesh_cluster against cluster_ref."""
    same(got[0], want[0], (what, "vertices"))
    same(got[1], want[1], (what, "faces"))
    close_normals(got[2], want[2], what)
    same(got[3], want[3], (what, "colors"))
    same(got[4], want[4], (what, "vertex_cluster"))


def same_mesh(mesh, want, what):
    assert isinstance(mesh, geometry.Mesh)
    same(mesh.vertices, want[0], (what, "vertices"))
    same(mesh.faces, want[1], (what, "faces"))
    close_normals(mesh.normals, want[2], what)
    same(mesh.colors, want[3], (what, "colors"))


def faces_are_sound(f, K):
    """Ids in [0, K), three different ids a face, the smallest first, no set of three twice."""
    f = np.asarray(f).reshape(-1, 3)
    if not len(f):
        return True
    sets = np.sort(f, axis=1)
    return bool(f.min() >= 0 and f.max() < K and (sets[:, 0] < sets[:, 1]).all() and (sets[:, 1] < sets[:, 2]).all()
                and (f[:, 0] == sets[:, 0]).all() and len(np.unique(sets, axis=0)) == len(f))


_COLORS = {}


def colors_of(name):
    if name not in _COLORS:
        c = np.random.default_rng(17).uniform(-0.05, 1.05, (len(C.mesh(name)[0]), 3)).astype(np.float32)      # a few outside [0, 1]: the clamp
        c.setflags(write=False)
        _COLORS[name] = c
    return _COLORS[name]


# ---------------------------------------------------------------- 1. hand cases
@pytest.mark.parametrize("name", sorted(S.HAND))
def test_hand_cases(name):
    case = S.hand(name)
    v, f, grid = case["v"], case["f"], (case["lo"], case["cell"], case["n"])
    rng = np.random.default_rng(len(v) + 1)
    nrm = rng.standard_normal((len(v), 3)).astype(np.float32)
    nrm /= np.maximum(np.linalg.norm(nrm, axis=1, keepdims=True), 1e-9).astype(np.float32)
    col = rng.uniform(0, 1, (len(v), 3)).astype(np.float32)
    want = S.cluster_ref(v, f, *grid, nrm, col)
    assert np.array_equal(want[4], case["vc"]) and np.array_equal(want[1], case["out_f"])
    assert faces_are_sound(want[1], len(want[0]))
    got = ops.mesh_cluster(dev(v), dev(f), *grid, normals=dev(nrm), colors=dev(col))
    same_cluster(got, want, name)
    for t, rows, dtype in ((got[0], len(want[0]), torch.float32), (got[1], len(want[1]), torch.int32), (got[4], len(v), torch.int32)):
        assert t.dtype == dtype and t.shape[0] == rows and t.is_contiguous() and t.device == torch.device(DEV)
    bare = ops.mesh_cluster(dev(v), dev(f), *grid)
    assert bare[2] is None and bare[3] is None
    same_cluster(bare, S.cluster_ref(v, f, *grid), (name, "bare"))
    if "out_v" in case:
        same(got[0], np.asarray(case["out_v"], np.float32).reshape(-1, 3), (name, "positions by hand"))


def test_everything_in_one_cell_and_nothing_merged():
    case = S.hand("everything in one cell")
    got = ops.mesh_cluster(dev(case["v"]), dev(case["f"]), case["lo"], case["cell"], case["n"])
    assert got[0].shape == (1, 3) and got[1].shape == (0, 3) and got[4].tolist() == [0, 0, 0, 0]
    case = S.hand("nothing merges")
    want = S.cluster_ref(case["v"], case["f"], case["lo"], case["cell"], case["n"])
    bound = 0.125 * 2.0 ** -20 + 2.0 ** -22          # the floor, and one float32 rounding of a coordinate below 2
    assert len(want[0]) == 4 and 0 < np.abs(want[0].astype(np.float64) - case["v"]).max() < bound
    mesh = geometry.Mesh(dev(case["v"]), dev(case["f"])).simplify(0.125, lo=(0, 0, 0), hi=(2, 2, 2))
    same_mesh(mesh, want, "nothing merges")
    assert mesh.vertices.shape[0] == 4 and float((mesh.vertices.cpu().double() - torch.from_numpy(case["v"]).double()).abs().max()) < bound
    assert mesh.faces.tolist() == [[0, 1, 2], [1, 3, 2]]          # equal to the input but for the rotation of the second


def test_an_empty_mesh_and_a_mesh_without_faces():
    empty = geometry.Mesh(torch.zeros(0, 3, device=DEV), torch.zeros(0, 3, dtype=torch.int32, device=DEV))
    got = empty.simplify(0.5)
    assert got.vertices.shape == (0, 3) and got.faces.shape == (0, 3) and got.normals is None and got.colors is None
    out = ops.mesh_cluster(empty.vertices, dev(np.array([[0, 1, 2]], np.int32)), (0, 0, 0), (1, 1, 1), (2, 2, 2), normals=empty.vertices)
    assert out[0].shape == (0, 3) and out[1].shape == (0, 3) and out[2].shape == (0, 3) and out[3] is None and out[4].shape == (0,)
    case = S.hand("no faces")
    dust = geometry.Mesh(dev(case["v"]), dev(case["f"]), None, dev(case["v"]))
    got = dust.simplify((1.0, 1.0, 1.0), lo=(0, 0, 0), hi=(2, 1, 1))
    assert got.faces.shape == (0, 3) and got.vertices.tolist() == [[.625, .5, .5], [1.5, .5, .5]] and got.normals is None
    assert got.colors.tolist() == [[.625, .5, .5], [1.0, .5, .5]]          # the members' colours clamped to [0, 1], then their mean


# ---------------------------------------------------------------- 2. blobs
@pytest.mark.parametrize("spacings", [2, 4])
def test_blobs_at_two_and_four_grid_spacings(spacings):
    v, f, n = C.mesh("blobs33")
    col = colors_of("blobs33")
    cell = spacings * 2.0 / 32
    lo, cells, nn = S.grid_of(v, cell, lo=(-1, -1, -1), hi=(1, 1, 1))
    assert nn == [32 // spacings] * 3
    d_v, d_f, d_n, d_c = dev(v), dev(f), dev(n), dev(col)
    sizes = {}
    for with_n, with_c in ((True, True), (True, False), (False, True), (False, False)):
        want = S.cluster_ref(v, f, lo, cells, nn, n if with_n else None, col if with_c else None)
        K = len(want[0])
        assert faces_are_sound(want[1], K) and 0 < K < len(v) // spacings and 0 < len(want[1]) < len(f) // spacings
        assert want[4].min() == 0 and want[4].max() == K - 1
        mesh = geometry.Mesh(d_v, d_f, d_n if with_n else None, d_c if with_c else None)
        got = mesh.simplify(cell, lo=(-1, -1, -1), hi=(1, 1, 1))
        same_mesh(got, want, ("blobs33", spacings, with_n, with_c))
        assert int(got.faces.min()) >= 0 and int(got.faces.max()) < K
        assert bool((got.faces[:, 0] == got.faces.min(dim=1).values).all())          # the smallest id first
        sizes[(with_n, with_c)] = (K, len(want[1]))
        # the original is untouched
        for t, w in ((mesh.vertices, v), (mesh.faces, f), (mesh.normals, n if with_n else None), (mesh.colors, col if with_c else None)):
            same(t, w, "original")
    assert len(set(sizes.values())) == 1          # normals and colours ride along: they change no vertex and no face
    print("blobs33 at %d spacings: %d vertices, %d faces -> %d, %d" % ((spacings, len(v), len(f)) + sizes[(True, True)]))
    # ops.mesh_cluster hands vertex_cluster back too; a per-axis cell size
    want = S.cluster_ref(v, f, (-1, -1, -1), (cell, 2 * cell, 0.3), (nn[0], nn[0] // 2, 7), n, col)
    same_cluster(ops.mesh_cluster(d_v, d_f, (-1, -1, -1), (cell, 2 * cell, 0.3), (nn[0], nn[0] // 2, 7), normals=d_n, colors=d_c), want, "per-axis")


# ---------------------------------------------------------------- 3. hot clusters
def test_hot_clusters_every_add_on_one_of_eight_addresses():
    v, f, n = C.mesh("noise41-0.6")
    col = colors_of("noise41-0.6")
    grid = ((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0), (2, 2, 2))
    vc, cc, m, Ssum, N, Csum = S.sums_ref(v, *grid, n, col)
    assert len(v) == 148181 and len(m) == 8 and m.min() > 15000 and m.sum() == len(v)
    want = S.cluster_ref(v, f, *grid, n, col)
    assert len(want[0]) == 8 and faces_are_sound(want[1], 8) and 0 < len(want[1]) <= 56          # at most C(8, 3) sets
    got = ops.mesh_cluster(dev(v), dev(f), *grid, normals=dev(n), colors=dev(col))
    same_cluster(got, want, "hot clusters")
    assert got[1].shape[0] == len(want[1])
    # the counts and the sums themselves: from the device's positions and colours back to the integers (exact: S / (m 2^20) has few digits)
    members = torch.bincount(got[4].long(), minlength=8).cpu().numpy()
    assert np.array_equal(members, m)
    back = np.rint((got[3].cpu().numpy().astype(np.float64) * (m[:, None] * 1048576.0))).astype(np.int64)
    assert np.abs(back - Csum).max() <= 1 + Csum.max() * 2.0 ** -24          # one float32 rounding of the mean, scaled back
    print("hot clusters: members %s, F' = %d" % (m.tolist(), len(want[1])))


# ---------------------------------------------------------------- 4. duplicate pressure
def _duplicates():
    """64 vertices, one per cell of a 4^3 grid, and 200,000 faces drawn from 40 sets of three of them, in both orientations, shuffled."""
    rng = np.random.default_rng(23)
    centres = np.stack(np.meshgrid(np.arange(4), np.arange(4), np.arange(4), indexing="ij"), axis=-1).reshape(-1, 3) + 0.5
    v = centres[rng.permutation(64)].astype(np.float32)
    sets = np.array([rng.choice(64, 3, replace=False) for _ in range(40)])
    pick = rng.integers(0, 40, 200000)
    f = sets[pick]
    roll = rng.integers(0, 3, 200000)
    f = np.stack([f[np.arange(200000), (roll + j) % 3] for j in range(3)], axis=1)
    flip = rng.random(200000) < 0.5
    f[flip] = f[flip][:, ::-1]
    return v, f.astype(np.int32), pick


def test_duplicate_pressure_the_smallest_index_of_every_set_is_kept():
    v, f, pick = _duplicates()
    grid = ((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (4, 4, 4))
    want = S.cluster_ref(v, f, *grid)
    assert len(want[0]) == 64 and want[4].tolist() == list(range(64))          # one vertex a cell: the cluster of a vertex is its id
    firsts = np.array(sorted(int(np.nonzero(pick == k)[0][0]) for k in range(40)))
    assert np.bincount(pick).min() > 4000 and len(want[1]) == 40 and faces_are_sound(want[1], 64)
    kept = f[firsts]
    roll = np.argmin(kept, axis=1)
    assert np.array_equal(want[1], np.stack([kept[np.arange(40), (roll + j) % 3] for j in range(3)], axis=1))
    got = ops.mesh_cluster(dev(v), dev(f), *grid)
    same_cluster(got, want, "duplicates")


# ---------------------------------------------------------------- 5. past the scan's chunk, a large table
def test_past_the_chunk_of_the_block_total_scan_and_a_large_table():
    v, f, n = C.mesh("noise73+0.35")
    assert (len(v), len(f)) == (1164962, 2391620) and len(v) > 1024 * 1024
    cell = 2 * 2.0 / 72
    lo, cells, nn = S.grid_of(v, cell, lo=(-1, -1, -1), hi=(1, 1, 1))
    assert nn == [36, 36, 36]
    col = colors_of("noise73+0.35")
    want = S.cluster_ref(v, f, lo, cells, nn, n, col)
    K = len(want[0])
    assert faces_are_sound(want[1], K) and 1024 < K <= 36 ** 3 and len(want[1]) > 1024
    mesh = geometry.Mesh(dev(v), dev(f), dev(n), dev(col)).simplify(cell, lo=(-1, -1, -1), hi=(1, 1, 1))
    same_mesh(mesh, want, "noise73")
    print("noise73+0.35 at 2 spacings: %d vertices, %d faces -> %d, %d" % (len(v), len(f), K, len(want[1])))


# ---------------------------------------------------------------- 6. determinism
def test_two_runs_give_equal_bytes_and_shuffled_faces_follow_the_restatement():
    v, f, n = C.mesh("noise41-0.6")
    col = colors_of("noise41-0.6")
    cell = 2 * 2.0 / 40
    mesh = geometry.Mesh(dev(v), dev(f), dev(n), dev(col))
    a, b = mesh.simplify(cell), mesh.simplify(cell)
    for name in ("vertices", "faces", "normals", "colors"):
        assert getattr(a, name).cpu().numpy().tobytes() == getattr(b, name).cpu().numpy().tobytes(), name
    lo, cells, nn = S.grid_of(v, cell)
    same_mesh(a, S.cluster_ref(v, f, lo, cells, nn, n, col), "bounding box")
    perm = np.random.default_rng(3).permutation(len(f))
    want = S.cluster_ref(v, f[perm], lo, cells, nn, n, col)
    assert faces_are_sound(want[1], len(want[0])) and not np.array_equal(want[1], S.cluster_ref(v, f, lo, cells, nn)[1])
    same_mesh(geometry.Mesh(mesh.vertices, dev(f[perm]), mesh.normals, mesh.colors).simplify(cell), want, "faces shuffled")


# ---------------------------------------------------------------- 7. plumbing
def test_emit_stops_at_the_capacities_and_null_normals_or_colours_leave_their_outputs():
    v, f, n = C.mesh("blobs33")
    col = colors_of("blobs33")
    grid = (-1.0, -1.0, -1.0, 0.125, 0.125, 0.125, 16, 16, 16)
    want = S.cluster_ref(v, f, grid[0:3], grid[3:6], grid[6:9], n, col)
    Vk, Fk = len(want[0]), len(want[1])
    lib = _lib.load()
    p = lambda t: ctypes.c_void_p(t.data_ptr())      # noqa: E731
    V, F = len(v), len(f)
    d_v, d_f, d_n, d_c = dev(v), dev(f), dev(n), dev(col)
    nbytes = lib.crnerf_mesh_cluster_workspace_bytes(V, F, 16 ** 3)
    ws = torch.full((nbytes + 64,), 0x5a, dtype=torch.uint8, device=DEV)          # a guard behind the workspace
    counts = torch.full((2,), -1, dtype=torch.int64, device=DEV)
    vc = torch.full((V + 1,), -7, dtype=torch.int32, device=DEV)
    st = _lib.stream_ptr()
    _lib.check(lib.crnerf_mesh_cluster_count_f32(p(d_v), p(d_f), V, F, *grid, p(ws), p(vc), p(counts), st), "count")
    assert counts.tolist() == [Vk, Fk] and int(vc[V]) == -7
    same(vc[:V], want[4], "vertex_cluster")

    def emit(v_cap, f_cap, with_normals=True, with_colors=True):
        ov, on, oc = (torch.full((Vk, 3), -7.0, device=DEV) for _ in range(3))
        of = torch.full((Fk, 3), -7, dtype=torch.int32, device=DEV)
        _lib.check(lib.crnerf_mesh_cluster_emit_f32(p(d_v), p(d_n) if with_normals else None, p(d_c) if with_colors else None, p(d_f), p(vc), V, F,
                                                    *grid, p(ws), v_cap, f_cap, p(ov), p(on), p(oc), p(of), st), "emit")
        return ov.cpu().numpy(), on.cpu().numpy(), oc.cpu().numpy(), of.cpu().numpy()
    # Vk and Fk rows each, the last one a guard: emit is told of Vk - 1 and Fk - 1
    ov, on, oc, of = emit(Vk - 1, Fk - 1)
    assert (ov[Vk - 1] == -7.0).all() and (on[Vk - 1] == -7.0).all() and (oc[Vk - 1] == -7.0).all() and (of[Fk - 1] == -7).all()
    assert np.array_equal(ov[:Vk - 1], want[0][:Vk - 1]) and np.array_equal(oc[:Vk - 1], want[3][:Vk - 1]) and np.array_equal(of[:Fk - 1], want[1][:Fk - 1])
    assert np.abs(on[:Vk - 1] - want[2][:Vk - 1]).max() <= NORMAL_TOL
    # far too short: the first rows, nothing else; no normals, no colours: their outputs are not touched
    ov, on, oc, of = emit(5, 3, with_normals=False, with_colors=False)
    assert (ov[5:] == -7.0).all() and (of[3:] == -7).all() and (on == -7.0).all() and (oc == -7.0).all()
    assert np.array_equal(ov[:5], want[0][:5]) and np.array_equal(of[:3], want[1][:3])
    ov, on, oc, of = emit(Vk, Fk, with_normals=False)
    assert (on == -7.0).all() and np.array_equal(oc, want[3]) and np.array_equal(ov, want[0])
    ov, on, oc, of = emit(Vk, Fk, with_colors=False)
    assert (oc == -7.0).all() and np.abs(on - want[2]).max() <= NORMAL_TOL
    ov, on, oc, of = emit(0, Fk)
    assert (ov == -7.0).all() and (on == -7.0).all() and (oc == -7.0).all() and np.array_equal(of, want[1])
    ov, on, oc, of = emit(Vk, 0)
    assert (of == -7).all() and np.array_equal(ov, want[0])
    ov, on, oc, of = emit(Vk, Fk)
    assert np.array_equal(ov, want[0]) and np.array_equal(oc, want[3]) and np.array_equal(of, want[1]) and np.abs(on - want[2]).max() <= NORMAL_TOL
    assert bool((ws[nbytes:] == 0x5a).all())          # nothing was written behind the workspace


def test_simplify_then_parts_largest_and_a_coloured_ply(tmp_path):
    v, f, n = C.mesh("blobs33")
    col = colors_of("blobs33")
    mesh = geometry.Mesh(dev(v), dev(f), dev(n), dev(col))
    small = mesh.simplify(0.125, lo=(-1, -1, -1), hi=(1, 1, 1))
    want = S.cluster_ref(v, f, (-1, -1, -1), (0.125,) * 3, (16, 16, 16), n, col)
    same_mesh(small, want, "small")
    ref = C.parts_ref(want[1], len(want[0]))
    parts = small.parts()
    assert parts.count == len(ref[2]) and parts.n_faces.tolist() == ref[3].tolist() and parts.vertex_part.tolist() == ref[0].tolist()
    big = small.largest()
    sel = C.select_ref(want[0], want[1], None, ref[0], ref[1], C.largest_ref(ref[3], 1))
    same(big.vertices, sel[0], "largest vertices")
    same(big.faces, sel[1], "largest faces")
    same(big.colors, want[3][ref[0] == int(np.argmax(ref[3]))], "largest colours")
    used = small.drop_small(1)          # the unused clusters go
    assert int(used.faces.max()) == used.vertices.shape[0] - 1 and len(np.unique(used.faces.cpu().numpy())) == used.vertices.shape[0]
    path = str(tmp_path / "small.ply")
    small.save_ply(path)
    with open(path, "rb") as fh:
        blob = fh.read()
    end = blob.index(b"end_header\n") + 11
    V, F = small.vertices.shape[0], small.faces.shape[0]
    head = blob[:end]
    assert b"element vertex %d\n" % V in head and b"element face %d\n" % F in head and b"property float nz\n" in head
    assert head.index(b"property uchar red\n") < head.index(b"property uchar green\n") < head.index(b"property uchar blue\n")
    rows = np.frombuffer(blob, dtype=np.dtype([("f", "<f4", (6,)), ("c", "u1", (3,))]), count=V, offset=end)
    tri = np.frombuffer(blob, dtype=np.dtype([("n", "u1"), ("i", "<i4", (3,))]), count=F, offset=end + 27 * V)
    assert end + 27 * V + 13 * F == len(blob) and (tri["n"] == 3).all()
    assert np.array_equal(rows["f"][:, :3], small.vertices.cpu().numpy()) and np.array_equal(rows["f"][:, 3:], small.normals.cpu().numpy())
    assert np.array_equal(rows["c"], (small.colors.clamp(0, 1) * 255).to(torch.uint8).cpu().numpy())
    assert np.array_equal(tri["i"], small.faces.cpu().numpy())


def test_the_bounding_box_default_equals_the_explicit_box():
    v, f, n = C.mesh("blobs33")
    mesh = geometry.Mesh(dev(v), dev(f), dev(n))
    lo, hi = v.min(axis=0).tolist(), v.max(axis=0).tolist()
    for cell in (0.125, (0.25, 0.1, 0.3)):
        a, b = mesh.simplify(cell), mesh.simplify(cell, lo=lo, hi=hi)
        for name in ("vertices", "faces", "normals"):
            assert torch.equal(getattr(a, name), getattr(b, name)), name
        assert a.colors is None and b.colors is None
        same_mesh(a, S.cluster_ref(v, f, *S.grid_of(v, cell), n), "bounding box")
        half = mesh.simplify(cell, lo=lo)
        assert torch.equal(half.vertices, a.vertices) and torch.equal(half.faces, a.faces)


class _Args:
    nerf_out_dim, img_wh = 64, [8, 8]


def test_extract_mesh_simplify_cell():
    m = NeRF_sigma("coarse", _Args(), in_channels_xyz=93, in_channels_dir=27).to(G.DEV)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in G.STATES[22].items()})
    m.eval()
    lo, hi, res = (-1.0, -0.5, 0.25), (1.0, 1.5, 2.0), (11, 6, 9)
    thr = float(geometry.density_grid(m, lo, hi, res).sigma.median())
    today = geometry.density_grid(m, lo, hi, res).mesh(thr)
    names = ("vertices", "faces", "normals")
    none = geometry.extract_mesh(m, lo, hi, res, thr, simplify_cell=None)
    for name in names:          # the default keeps today's result byte for byte
        assert getattr(none, name).cpu().numpy().tobytes() == getattr(today, name).cpu().numpy().tobytes(), name
        assert torch.equal(getattr(geometry.extract_mesh(m, lo, hi, res, thr), name), getattr(today, name)), name
    assert none.colors is None
    for c in (0.5, (0.45, 0.8, 0.4)):
        got, want = geometry.extract_mesh(m, lo, hi, res, thr, simplify_cell=c), today.simplify(c)
        kept, big = geometry.extract_mesh(m, lo, hi, res, thr, keep_largest=True, simplify_cell=c), today.largest().simplify(c)
        for name in names:
            assert torch.equal(getattr(got, name), getattr(want, name)), name
            assert torch.equal(getattr(kept, name), getattr(big, name)), name
        assert 0 < got.vertices.shape[0] < today.vertices.shape[0]
        # against the restatement, from the device's own mesh
        v, f, n = (t.cpu().numpy() for t in (today.vertices, today.faces, today.normals))
        same_mesh(got, S.cluster_ref(v, f, *S.grid_of(v, c), n), ("extract_mesh", c))

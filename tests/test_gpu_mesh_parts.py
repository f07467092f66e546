"""GPU checks of the mesh parts (include/crnerf_mesh_parts.h, ops.mesh_parts / mesh_select, crnerf_amd.geometry.Mesh.parts / select / largest /
drop_small): connected components and floater removal on the device.  Every comparison is bit for bit against the NumPy restatement
(tests/_mesh_parts_cases.py); the meshes come from the restatement of crnerf_mesh.h, so nothing here rests on csrc/mesh.hip but test 7.

  1. Hand cases.   2. blobs(33): six parts, one open, a cavity whose ids interleave with its outer surface.   3. A tie in the face counts.
  4. One long part (a helical tube).   5. Many parts: 2,824 (no giant part) and 1,427 (near percolation: the hard case for the union).
  6. Past the chunk of the block-total scan: 1,164,962 vertices (> 1,024 x 1,024), 2,391,620 faces, 2,366,254 of them in one part.
  7. Determinism and plumbing: equal bytes, capacities with a guard row, labels outside [0, K), extract_mesh(keep_largest=), PLY.

The helical tube is built in closed form (the centre-line point at the node's own angle on every turn): V 49,696, F 99,388, K = 1.
"""
import ctypes

import numpy as np
import pytest
import torch

from crnerf_amd import _lib, geometry, ops
from crnerf_amd.models.nerf import NeRF_sigma

import _geometry_cases as G
import _mesh_cases as M
import _mesh_parts_cases as C

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


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


def label(faces, V):
    vp, fp, pv, pf = ops.mesh_parts(dev(faces), V)
    for t, n in ((vp, V), (fp, len(faces)), (pv, pf.shape[0]), (pf, pv.shape[0])):
        assert t.dtype == torch.int32 and t.dim() == 1 and t.shape[0] == n and t.is_contiguous() and t.device == torch.device(DEV)
    return vp, fp, pv, pf


def same_parts(got, want, what):
    for g, w, n in zip(got, want, ("vertex_part", "face_part", "part_vertices", "part_faces")):
        same(g, w, (what, n))


def same_mesh(mesh, want, what):
    assert isinstance(mesh, geometry.Mesh)
    assert mesh.vertices.shape[1:] == (3,) and mesh.faces.shape[1:] == (3,)
    same(mesh.vertices, want[0], (what, "vertices"))
    same(mesh.faces, want[1], (what, "faces"))
    same(mesh.normals, want[2], (what, "normals"))


_ON_DEVICE = {}


def case(name, normals=True):
    """(Mesh on the device, (v, f, n) on the host, parts_ref) of a named field; uploaded once."""
    if name not in _ON_DEVICE:
        v, f, n = C.mesh(name)
        _ON_DEVICE[name] = geometry.Mesh(dev(v), dev(f), dev(n))
    m = _ON_DEVICE[name]
    v, f, n = C.mesh(name)
    if not normals:
        return geometry.Mesh(m.vertices, m.faces, None), (v, f, None), C.parts(name)
    return m, (v, f, n), C.parts(name)


def check_labels(name):
    mesh, (v, f, n), ref = case(name)
    parts = mesh.parts()
    assert isinstance(parts, geometry.MeshParts) and parts.count == len(ref[2])
    same_parts((parts.vertex_part, parts.face_part, parts.n_vertices, parts.n_faces), ref, name)
    return mesh, (v, f, n), ref, parts


# ---------------------------------------------------------------- 1. hand cases
@pytest.mark.parametrize("name", sorted(C.HAND))
def test_hand_cases(name):
    f, V, vp, fp = C.hand(name)
    ref = C.parts_ref(f, V)
    assert np.array_equal(ref[0], vp) and np.array_equal(ref[1], fp)
    got = label(f, V)
    same_parts(got, ref, name)
    K = len(ref[2])
    v = np.random.default_rng(V).standard_normal((V, 3)).astype(np.float32)
    nrm = -v
    for keep in [np.ones(K, np.uint8), np.zeros(K, np.uint8)] + [(np.arange(K) == k).astype(np.uint8) for k in range(K)]:
        out = ops.mesh_select(dev(v), dev(f), dev(nrm), got[0], got[1], dev(keep))
        want = C.select_ref(v, f, nrm, vp, fp, keep)
        for g, w, n in zip(out, want, "vfn"):
            same(g, w, (name, keep.tolist(), n))
        assert out[1].numel() == 0 or (0 <= int(out[1].min()) and int(out[1].max()) < out[0].shape[0])


def test_bad_ids_are_part_minus_one_and_never_emitted():
    f, V, vp, fp = C.hand("bad ids")
    got = label(f, V)
    assert got[1].tolist() == [0, -1, 1, -1, 1] and got[0].tolist() == [0, 0, 0, 1, 1, 1] and got[3].tolist() == [1, 2]
    out = ops.mesh_select(torch.zeros(V, 3, device=DEV), dev(f), None, got[0], got[1], torch.ones(2, dtype=torch.bool, device=DEV))
    assert out[1].tolist() == [[0, 1, 2], [3, 4, 5], [4, 5, 3]] and out[2] is None


# ---------------------------------------------------------------- 2. blobs
def test_blobs_labels_sizes_and_every_way_to_select():
    mesh, (v, f, n), ref, parts = check_labels("blobs33")
    vp, fp, pv, pf = ref
    assert (len(v), len(f), parts.count) == (4272, 8490, 6) and parts.n_faces.tolist() == [434, 5796, 632, 408, 1104, 116]
    # largest(): part 1, closed, its rows the original rows at the kept ids
    big = mesh.largest()
    same_mesh(big, C.select_ref(v, f, n, vp, fp, C.largest_ref(pf, 1)), "largest")
    kept = np.nonzero(vp == 1)[0]
    same(big.vertices, v[kept], "rows")
    same(big.normals, n[kept], "normal rows")
    assert big.faces.shape[0] == 5796
    t = M.topology(big.faces.cpu().numpy(), big.vertices.shape[0])
    assert t["uses"] == {2: t["E"]} and t["directed_max"] == 1 and t["chi"] == 2 and t["unused"] == 0
    assert bool((big.faces[:, 0] == big.faces.min(dim=1).values).all())          # "smallest id first" survives the monotone renumbering
    # the original is untouched
    same_mesh(mesh, (v, f, n), "original")
    same_mesh(mesh.largest(2), C.select_ref(v, f, n, vp, fp, C.largest_ref(pf, 2)), "largest(2)")      # the outer surface and the far sphere
    assert C.largest_ref(pf, 2).tolist() == [0, 1, 0, 0, 1, 0]
    same_mesh(mesh.largest(2, parts=parts), C.select_ref(v, f, n, vp, fp, C.largest_ref(pf, 2)), "largest(2, parts)")
    same_mesh(mesh.largest(99), (v, f, n), "largest(99)")
    same_mesh(mesh.largest(0), C.select_ref(v, f, n, vp, fp, np.zeros(6)), "largest(0)")
    same_mesh(mesh.drop_small(500), C.select_ref(v, f, n, vp, fp, pf >= 500), "drop_small(500)")
    assert (pf >= 500).tolist() == [False, True, True, False, True, False]
    by_ids = mesh.select([4, 1, 1], parts=parts)
    mask = np.array([0, 1, 0, 0, 1, 0], np.uint8)
    same_mesh(by_ids, C.select_ref(v, f, n, vp, fp, mask), "select by ids")
    for keep in (dev(mask), dev(mask.astype(bool)), torch.from_numpy(mask)):
        got = mesh.select(keep)
        for a in ("vertices", "faces", "normals"):
            assert torch.equal(getattr(got, a), getattr(by_ids, a)), a
    # the cavity alone: its ids lie strictly inside the outer surface's id range
    same_mesh(mesh.select([2]), C.select_ref(v, f, n, vp, fp, np.arange(6) == 2), "the cavity")
    # no normals: None stays None
    bare, want, _ = case("blobs33", normals=False)
    got = bare.largest()
    assert got.normals is None
    same_mesh(got, C.select_ref(v, f, None, vp, fp, C.largest_ref(pf, 1)), "largest, no normals")
    for bad in ([6], torch.zeros(5, dtype=torch.bool, device=DEV), torch.zeros(6, dtype=torch.int32, device=DEV)):
        with pytest.raises(ValueError):
            mesh.select(bad)


def test_blobs_17_lose_the_smallest_floater():
    _, _, ref, parts = check_labels("blobs17")
    assert parts.count == 5


# ---------------------------------------------------------------- 3. a tie
def test_a_tie_goes_to_the_smaller_part_id():
    mesh, (v, f, n), ref, parts = check_labels("tie")
    assert parts.n_faces.tolist() == [3456, 3456]
    same_mesh(mesh.largest(), C.select_ref(v, f, n, ref[0], ref[1], [1, 0]), "tie")
    assert int(mesh.largest().faces.shape[0]) == 3456 and torch.equal(mesh.largest().vertices, mesh.select([0]).vertices)


# ---------------------------------------------------------------- 4. a long part
def test_a_helical_tube_is_one_part():
    mesh, (v, f, n), ref, parts = check_labels("helix")
    assert (len(v), len(f), parts.count) == (49696, 99388, 1)
    assert parts.n_faces.tolist() == [99388] and parts.n_vertices.tolist() == [49696]
    same_mesh(mesh.largest(), (v, f, n), "the whole tube")


# ---------------------------------------------------------------- 5. many parts
@pytest.mark.parametrize("name,V,F,K,largest", [("noise41-0.75", 102424, 189232, 2824, 1744), ("noise41-0.6", 148181, 285554, 1427, 175964)])
def test_many_parts(name, V, F, K, largest):
    mesh, (v, f, n), ref, parts = check_labels(name)
    vp, fp, pv, pf = ref
    assert (len(v), len(f), parts.count, int(parts.n_faces.max())) == (V, F, K, largest)
    same_mesh(mesh.largest(3, parts=parts), C.select_ref(v, f, n, vp, fp, C.largest_ref(pf, 3)), "largest(3)")
    same_mesh(mesh.drop_small(8, parts=parts), C.select_ref(v, f, n, vp, fp, pf >= 8), "drop_small(8)")
    # ties among tiny parts: the first cut of the ranking, past 3, that falls inside a run of equal sizes
    order = sorted(range(K), key=lambda k: (-int(pf[k]), k))
    cut = next(c for c in range(4, K) if pf[order[c - 1]] == pf[order[c]])
    print("%s: largest(%d) cuts a run of parts with %d faces" % (name, cut, pf[order[cut]]))
    same_mesh(mesh.largest(cut, parts=parts), C.select_ref(v, f, n, vp, fp, C.largest_ref(pf, cut)), "largest(%d)" % cut)


# ---------------------------------------------------------------- 6. past the scan's chunk
def test_past_the_chunk_of_the_block_total_scan():
    mesh, (v, f, n), ref, parts = check_labels("noise73+0.35")
    vp, fp, pv, pf = ref
    assert (len(v), len(f), parts.count) == (1164962, 2391620, 921) and len(v) > 1024 * 1024
    assert int(parts.n_faces.max()) == 2366254 and int(parts.n_faces.sum()) == len(f)
    same_mesh(mesh.largest(parts=parts), C.select_ref(v, f, n, vp, fp, C.largest_ref(pf, 1)), "largest")
    same_mesh(mesh.drop_small(100, parts=parts), C.select_ref(v, f, n, vp, fp, pf >= 100), "drop_small(100)")
    # the floaters alone: the kept rows are sparse in every block
    same_mesh(mesh.select(parts.n_faces < 2366254, parts=parts), C.select_ref(v, f, n, vp, fp, pf < 2366254), "the floaters")


# ---------------------------------------------------------------- 7. determinism and plumbing
def test_two_runs_give_equal_bytes():
    mesh, (v, f, n), ref = case("noise41-0.6")
    a, b = mesh.parts(), mesh.parts()
    for name in ("vertex_part", "face_part", "n_vertices", "n_faces"):
        assert getattr(a, name).cpu().numpy().tobytes() == getattr(b, name).cpu().numpy().tobytes(), name
    x, y = mesh.drop_small(8), mesh.drop_small(8)
    for name in ("vertices", "faces", "normals"):
        assert getattr(x, name).cpu().numpy().tobytes() == getattr(y, name).cpu().numpy().tobytes(), name
    # the order of the faces is not what the labels rest on
    perm = np.random.default_rng(3).permutation(len(f))
    got = label(f[perm], len(v))
    same(got[0], ref[0], "vertex_part, faces shuffled")
    same(got[1], ref[1][perm], "face_part, faces shuffled")


def test_emit_stops_at_the_capacities():
    mesh, (v, f, n), ref = case("blobs33")
    vp, fp, pv, pf = ref
    keep = np.array([0, 1, 0, 1, 1, 0], np.uint8)
    want = C.select_ref(v, f, n, vp, fp, keep)
    Vk, Fk = len(want[0]), len(want[1])
    lib = _lib.load()
    p = lambda t: ctypes.c_void_p(t.data_ptr())      # noqa: E731
    V, F, K = len(v), len(f), 6
    ws = torch.empty(lib.crnerf_mesh_parts_workspace_bytes(V, F), dtype=torch.uint8, device=DEV)
    counts = torch.full((2,), -1, dtype=torch.int64, device=DEV)
    d_vp, d_fp, d_keep = dev(vp), dev(fp), dev(keep)
    st = _lib.stream_ptr()
    _lib.check(lib.crnerf_mesh_parts_select_count(p(d_vp), p(d_fp), V, F, K, p(d_keep), p(ws), p(counts), st), "select_count")
    assert counts.tolist() == [Vk, Fk]

    def emit(v_cap, f_cap, with_normals=True):
        ov, on = torch.full((Vk, 3), -7.0, device=DEV), torch.full((Vk, 3), -7.0, device=DEV)
        of = torch.full((Fk, 3), -7, dtype=torch.int32, device=DEV)
        _lib.check(lib.crnerf_mesh_parts_select_emit_f32(p(mesh.vertices), p(mesh.normals) if with_normals else None, p(mesh.faces), p(d_vp), p(d_fp),
                                                         V, F, K, p(d_keep), p(ws), v_cap, f_cap, p(ov), p(on), p(of), st), "select_emit")
        return ov.cpu().numpy(), on.cpu().numpy(), of.cpu().numpy()
    # Vk and Fk rows each, the last one a guard: emit is told of Vk - 1 and Fk - 1
    ov, on, of = emit(Vk - 1, Fk - 1)
    assert (ov[Vk - 1] == -7.0).all() and (on[Vk - 1] == -7.0).all() and (of[Fk - 1] == -7).all()
    assert np.array_equal(ov[:Vk - 1], want[0][:Vk - 1]) and np.array_equal(on[:Vk - 1], want[2][:Vk - 1]) and np.array_equal(of[:Fk - 1], want[1][:Fk - 1])
    # far too short: the first rows, nothing else; no normals: out_normals is not touched
    ov, on, of = emit(5, 3, with_normals=False)
    assert (ov[5:] == -7.0).all() and (of[3:] == -7).all() and (on == -7.0).all()
    assert np.array_equal(ov[:5], want[0][:5]) and np.array_equal(of[:3], want[1][:3])
    ov, on, of = emit(0, Fk)
    assert (ov == -7.0).all() and np.array_equal(of, want[1])
    ov, on, of = emit(Vk, Fk)
    assert np.array_equal(ov, want[0]) and np.array_equal(on, want[2]) and np.array_equal(of, want[1])


def test_labels_outside_the_parts_count_as_not_kept_and_are_not_counted():
    mesh, (v, f, n), ref = case("blobs33")
    vp, fp = ref[0].copy(), ref[1].copy()
    rng = np.random.default_rng(11)
    fp[rng.choice(len(fp), 300, replace=False)] = rng.choice([-1, -5, 6, 7, 2 ** 31 - 1, -2 ** 31], 300)
    lone = np.nonzero(ref[0] == 3)[0]
    vp[lone] = rng.choice([-1, 6, 2 ** 31 - 1, -2 ** 31], len(lone))      # a whole part's vertices (its faces are still labelled 3: dropped by keep)
    keep = np.array([1, 1, 1, 0, 1, 1], np.uint8)
    out = ops.mesh_select(mesh.vertices, mesh.faces, mesh.normals, dev(vp), dev(fp), dev(keep))
    want = C.select_ref(v, f, n, vp, fp, keep)
    for g, w, name in zip(out, want, "vfn"):
        same(g, w, name)
    lib = _lib.load()
    p = lambda t: ctypes.c_void_p(t.data_ptr())      # noqa: E731
    pv, pf = torch.full((6,), -9, dtype=torch.int32, device=DEV), torch.full((6,), -9, dtype=torch.int32, device=DEV)
    d_vp, d_fp = dev(vp), dev(fp)
    _lib.check(lib.crnerf_mesh_parts_sizes_i32(p(d_vp), p(d_fp), len(v), len(f), 6, p(pv), p(pf), _lib.stream_ptr()), "sizes")
    assert pv.tolist() == [int(((vp == k)).sum()) for k in range(6)] and pf.tolist() == [int((fp == k).sum()) for k in range(6)]
    assert pv.tolist()[3] == 0


def test_an_empty_mesh_and_a_mesh_without_faces():
    empty = geometry.Mesh(torch.zeros(0, 3, device=DEV), torch.zeros(0, 3, dtype=torch.int32, device=DEV), None)
    parts = empty.parts()
    assert parts.count == 0 and parts.vertex_part.shape == (0,) and parts.face_part.shape == (0,)
    for got in (empty.largest(), empty.drop_small(1), empty.select([]), empty.select(torch.zeros(0, dtype=torch.bool))):
        assert got.vertices.shape == (0, 3) and got.faces.shape == (0, 3) and got.normals is None
    v = torch.arange(15, dtype=torch.float32, device=DEV).reshape(5, 3)
    dust = geometry.Mesh(v, torch.zeros(0, 3, dtype=torch.int32, device=DEV), -v)
    parts = dust.parts()
    assert parts.count == 5 and parts.vertex_part.tolist() == [0, 1, 2, 3, 4] and parts.n_vertices.tolist() == [1] * 5 and parts.n_faces.tolist() == [0] * 5
    got = dust.largest()                           # all sizes tie at 0: part 0
    assert torch.equal(got.vertices, v[:1]) and torch.equal(got.normals, -v[:1]) and got.faces.shape == (0, 3)
    got = dust.select([3, 1])
    assert torch.equal(got.vertices, v[[1, 3]])
    assert dust.drop_small(1).vertices.shape == (0, 3) and torch.equal(dust.drop_small(0).vertices, v)


class _Args:
    nerf_out_dim, img_wh = 64, [8, 8]


def test_extract_mesh_keep_largest_and_ply_round_trip(tmp_path):
    m = NeRF_sigma("coarse", _Args(), in_channels_xyz=93, in_channels_dir=27).to(G.DEV)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in G.STATES[22].items()})
    m.eval()
    lo, hi, res = (-1.0, -0.5, 0.25), (1.0, 1.5, 2.0), (11, 6, 9)
    dg = geometry.density_grid(m, lo, hi, res)
    thr = float(dg.sigma.median())
    today = dg.mesh(thr)
    plain, default, kept = geometry.extract_mesh(m, lo, hi, res, thr, keep_largest=False), geometry.extract_mesh(m, lo, hi, res, thr), \
        geometry.extract_mesh(m, lo, hi, res, thr, keep_largest=True)
    big = today.largest()
    for name in ("vertices", "faces", "normals"):
        assert torch.equal(getattr(plain, name), getattr(today, name)) and torch.equal(getattr(default, name), getattr(today, name)), name
        assert torch.equal(getattr(kept, name), getattr(big, name)), name
    # against the restatement, from the device's own mesh
    v, f, n = (t.cpu().numpy() for t in (today.vertices, today.faces, today.normals))
    ref = C.parts_ref(f, len(v))
    same_mesh(kept, C.select_ref(v, f, n, ref[0], ref[1], C.largest_ref(ref[3], 1)), "keep_largest")
    # PLY of a selected mesh
    sel = case("blobs33")[0].drop_small(500)
    path = str(tmp_path / "parts.ply")
    sel.save_ply(path)
    with open(path, "rb") as fh:
        blob = fh.read()
    end = blob.index(b"end_header\n") + 11
    V, F = sel.vertices.shape[0], sel.faces.shape[0]
    assert b"element vertex %d\n" % V in blob[:end] and b"element face %d\n" % F in blob[:end] and b"property float nz\n" in blob[:end]
    rows = np.frombuffer(blob, dtype="<f4", count=6 * V, offset=end).reshape(V, 6)
    tri = np.frombuffer(blob, dtype=np.dtype([("n", "u1"), ("i", "<i4", (3,))]), count=F, offset=end + 24 * V)
    assert end + 24 * V + 13 * F == len(blob) and (tri["n"] == 3).all()
    assert np.array_equal(rows[:, :3], sel.vertices.cpu().numpy()) and np.array_equal(rows[:, 3:], sel.normals.cpu().numpy())
    assert np.array_equal(tri["i"], sel.faces.cpu().numpy()) and tri["i"].max() == V - 1

"""Host-side checks of the mesh parts (include/crnerf_mesh_parts.h, ops.mesh_parts / mesh_select, crnerf_amd.geometry.Mesh.parts / select / largest /
drop_small; no GPU needed): the header against its table of _lib.HEADER_SIGNATURES, the exports, every refusal and every no-op of the entries --
each call below is refused, or does nothing, on the host before any device work, so the pointers are never followed --, the ValueErrors of the
geometry layer, and the NumPy restatement the GPU tests compare with (tests/_mesh_parts_cases.py) held to hand cases and to scipy's connected
components."""
import importlib.util
import os

import numpy as np
import pytest
import torch

from crnerf_amd import _lib, geometry, ops

import _abi
from _abi import bound as _fn, header_text as _header, last_error as _last_error
import _mesh_cases as M
import _mesh_parts_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 4096          # a non-NULL, 16-byte aligned pointer that is never followed
BIG = 2 ** 31 - 1
BYTES, LABEL, SIZES = "crnerf_mesh_parts_workspace_bytes", "crnerf_mesh_parts_label_i32", "crnerf_mesh_parts_sizes_i32"
COUNT, EMIT = "crnerf_mesh_parts_select_count", "crnerf_mesh_parts_select_emit_f32"
SHAPE, NULL, CONFIG = -2, -1, -3          # CRNERF_ERR_*
TABLE = _lib.HEADER_SIGNATURES["crnerf_mesh_parts.h"]


def test_header_declares_the_five_entries_and_matches_the_signature_table():
    _abi.check_header("crnerf_mesh_parts.h")            # every return type and every parameter, by C type
    protos = _abi.prototypes("crnerf_mesh_parts.h")
    assert list(protos) == list(TABLE) == [BYTES, LABEL, SIZES, COUNT, EMIT]
    assert [len(protos[n][1]) for n in (BYTES, LABEL, SIZES, COUNT, EMIT)] == [2, 8, 8, 9, 16]
    # in no other header's table (tests/test_host.py: pairwise disjoint, 152 rows in all); the older headers do not know the entries
    assert not set(TABLE) & set().union(*(t for h, t in _lib.HEADER_SIGNATURES.items() if h != "crnerf_mesh_parts.h"))
    for older in ("crnerf.h", "crnerf_geometry.h", "crnerf_mesh.h"):
        assert "crnerf_mesh_parts_" not in _header(older)


def test_header_states_the_rules():
    text = _header("crnerf_mesh_parts.h")
    for word in ("Valid face.", "Parts.", "Part ids.", "Labels.", "Sizes.", "Selection", "Kept vertices", "Kept faces", "Largest.", "never dereferenced",
                 "ascending in the smallest vertex id", "ties to the smaller part id", "one cycle", "same bytes on every run", "byte copies",
                 "face_part = -1", "outside [0, K)"):
        assert word in text, word


def test_build_and_entry_know_the_unit_and_the_header():
    spec = importlib.util.spec_from_file_location("crnerf_build_for_mesh_parts", os.path.join(ROOT, "cr-nerf-pytorch_amd", "build.py"))
    build = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(build)
    assert "mesh_parts.hip" in build.SOURCES and all("../../include/" + header in build.HEADERS for header in _lib.HEADER_SIGNATURES)
    import __graft_entry__ as entry                         # the missing-symbol check covers this header's table
    assert set(entry.missing_symbols(object())) >= set(TABLE)


NEGATIVE = ((-1, 4), (4, -1), (-1, -1), (-2 ** 63, 0))
TOO_MANY = ((2 ** 31, 4), (4, 2 ** 31), (2 ** 40, 2 ** 40), (2 ** 63 - 1, 1))
WORK = ((1, 0), (5, 0), (3, 1), (BIG, BIG), (4, BIG))


def test_label_refuses_before_any_device_work():
    fn = _fn(LABEL)
    who = b"mesh_parts_label: "
    for V, F in NEGATIVE:
        assert fn(P, V, F, P, P, P, P, None) == SHAPE, (V, F)
        assert _last_error() == who + b"negative size"
    for V, F in TOO_MANY:
        assert fn(P, V, F, P, P, P, P, None) == SHAPE, (V, F)
        assert _last_error().startswith(who + b"more than 2^31 - 1")
    for F in (0, 7, BIG):                                       # no vertex: nothing to do, nothing is looked at (counts NULL: nowhere to write the zero)
        assert fn(None, 0, F, None, None, None, None, None) == 0
        assert fn(P, 0, F, P + 8, P, P, None, None) == 0
    for V, F in WORK:
        for k, field in ((0, b"faces"), (3, b"workspace"), (4, b"vertex_part"), (5, b"face_part"), (6, b"counts")):
            a = [P, V, F, P, P, P, P, None]
            a[k] = None
            if F == 0 and field in (b"faces", b"face_part"):    # no face: neither is needed; the call gets as far as the alignment check
                a[3] = P + 8
                assert fn(*a) == CONFIG, (field, V, F)
                continue
            assert fn(*a) == NULL, (field, V, F)
            assert _last_error() == who + field + b" is NULL"
        assert fn(P, V, F, P + 8, P, P, P, None) == CONFIG
        assert _last_error() == who + b"workspace must be 16-byte aligned"


def test_sizes_refuses_before_any_device_work():
    fn = _fn(SIZES)
    who = b"mesh_parts_sizes: "
    for V, F in NEGATIVE:
        assert fn(P, P, V, F, 1, P, P, None) == SHAPE and _last_error() == who + b"negative size"
    assert fn(P, P, 4, 4, -1, P, P, None) == SHAPE and _last_error() == who + b"negative size"
    for V, F in TOO_MANY:
        assert fn(P, P, V, F, 1, P, P, None) == SHAPE and _last_error().startswith(who + b"more than 2^31 - 1")
    for V, K in ((4, 5), (0, 1), (BIG, 2 ** 31)):
        assert fn(P, P, V, 4, K, P, P, None) == SHAPE and _last_error().startswith(who + b"more parts than vertices")
    assert fn(None, None, 0, 0, 0, None, None, None) == 0       # no vertex
    assert fn(None, None, 0, 9, 0, None, None, None) == 0
    assert fn(None, None, 9, 9, 0, None, None, None) == 0       # no part
    for k, field in ((0, b"vertex_part"), (1, b"face_part"), (5, b"part_vertices"), (6, b"part_faces")):
        a = [P, P, 4, 4, 2, P, P, None]
        a[k] = None
        assert fn(*a) == NULL and _last_error() == who + field + b" is NULL"


def test_select_count_refuses_before_any_device_work():
    fn = _fn(COUNT)
    who = b"mesh_parts_select_count: "
    for V, F in NEGATIVE:
        assert fn(P, P, V, F, 1, P, P, P, None) == SHAPE and _last_error() == who + b"negative size"
    assert fn(P, P, 4, 4, -1, P, P, P, None) == SHAPE and _last_error() == who + b"negative size"
    for V, F in TOO_MANY:
        assert fn(P, P, V, F, 1, P, P, P, None) == SHAPE and _last_error().startswith(who + b"more than 2^31 - 1")
    assert fn(P, P, 4, 4, 5, P, P, P, None) == SHAPE and _last_error().startswith(who + b"more parts than vertices")
    assert fn(None, None, 0, 0, 0, None, None, None, None) == 0
    assert fn(None, None, 0, 9, 0, None, P + 4, None, None) == 0
    for V, F in WORK:
        for k, field in ((0, b"vertex_part"), (1, b"face_part"), (5, b"keep"), (6, b"workspace"), (7, b"counts")):
            a = [P, P, V, F, 1, P, P, P, None]
            a[k] = None
            if F == 0 and field == b"face_part":
                a[6] = P + 8
                assert fn(*a) == CONFIG
                continue
            assert fn(*a) == NULL, (field, V, F)
            assert _last_error() == who + field + b" is NULL"
        assert fn(P, P, V, F, 1, P, P + 2, P, None) == CONFIG
        assert _last_error() == who + b"workspace must be 16-byte aligned"


def test_select_emit_refuses_before_any_device_work():
    fn = _fn(EMIT)
    who = b"mesh_parts_select_emit: "

    def call(V=4, F=4, K=2, v_cap=8, f_cap=8, vertices=P, normals=P, faces=P, vertex_part=P, face_part=P, keep=P, workspace=P, out_vertices=P,
             out_normals=P, out_faces=P):
        return fn(vertices, normals, faces, vertex_part, face_part, V, F, K, keep, workspace, v_cap, f_cap, out_vertices, out_normals, out_faces, None)
    for V, F in NEGATIVE:
        assert call(V, F) == SHAPE and _last_error() == who + b"negative size"
    assert call(K=-1) == SHAPE and _last_error() == who + b"negative size"
    for V, F in TOO_MANY:
        assert call(V, F) == SHAPE and _last_error().startswith(who + b"more than 2^31 - 1")
    assert call(K=5) == SHAPE and _last_error().startswith(who + b"more parts than vertices")
    for caps in ((2 ** 31, 8), (8, 2 ** 31), (2 ** 40, 2 ** 40), (2 ** 63 - 1, 0)):
        assert call(BIG, BIG, 1, *caps) == SHAPE and _last_error().startswith(who + b"a capacity above 2^31 - 1")
    for caps in ((-1, 8), (8, -1)):
        assert call(4, 4, 2, *caps) == SHAPE and _last_error() == who + b"negative capacity"
    nothing = dict(vertices=None, normals=None, faces=None, vertex_part=None, face_part=None, keep=None, workspace=None, out_vertices=None,
                   out_normals=None, out_faces=None)
    assert call(0, 0, 0, **nothing) == 0 and call(0, 9, 0, BIG, BIG, **nothing) == 0          # no vertex
    assert call(9, 9, 0, **nothing) == 0                                                       # no part: nothing is kept
    assert call(9, 9, 3, 0, 0, **nothing) == 0                                                 # room for nothing
    assert call(9, 0, 3, 0, 8, **nothing) == 0                                                 # room for faces only, and there are none
    for field in ("vertices", "faces", "vertex_part", "face_part", "keep", "workspace", "out_vertices", "out_normals", "out_faces"):
        for V, F in ((4, 4), (BIG, BIG)):
            assert call(V, F, 1, BIG, BIG, **{field: None}) == NULL, field
            assert _last_error() == who + field.encode() + b" is NULL"
    assert call(normals=None, out_normals=None, workspace=P + 8) == CONFIG                     # no normals: out_normals is not needed
    assert call(v_cap=0, vertices=None, out_vertices=None, out_normals=None, workspace=P + 8) == CONFIG      # faces only
    assert call(f_cap=0, faces=None, face_part=None, out_faces=None, workspace=P + 8) == CONFIG              # vertices only
    assert call(F=0, faces=None, face_part=None, out_faces=None, workspace=P + 8) == CONFIG
    assert _last_error() == who + b"workspace must be 16-byte aligned"


def test_workspace_bytes_is_monotone_and_zero_for_no_vertex():
    fn = _fn(BYTES)
    for V, F in ((0, 0), (0, 9), (-1, 4), (4, -1)) + TOO_MANY:
        assert fn(V, F) == 0, (V, F)
    assert fn(1, 0) > 0
    for V, F in ((1, 0), (5, 7), (1024, 1024), (4272, 8490)):
        for step in (1, 2, 7, 1000):
            assert fn(V + step, F) > fn(V, F) and fn(V, F + step) > fn(V, F)
    assert fn(BIG, BIG) >= 6 * BIG + 2 * BIG           # parent and a 16-bit offset per vertex, a 16-bit offset per face


# ---------------------------------------------------------------- the Python layer
def _cpu_mesh():
    f, V, _, _ = C.hand("two disjoint triangles")
    return geometry.Mesh(torch.zeros(V, 3), torch.from_numpy(f), None)


def _cpu_parts():
    _, _, vp, fp = C.hand("two disjoint triangles")
    return geometry.MeshParts(torch.from_numpy(vp), torch.from_numpy(fp), torch.tensor([3, 3], dtype=torch.int32), torch.tensor([1, 1], dtype=torch.int32))


def test_the_geometry_layer_refuses_a_bad_keep():
    mesh, parts = _cpu_mesh(), _cpu_parts()
    assert parts.count == 2
    # dtype and rank: before the parts are asked for (parts=None would need the device)
    with pytest.raises(ValueError, match="bool or uint8 tensor"):
        mesh.select(torch.zeros(2, dtype=torch.float32))
    with pytest.raises(ValueError, match="bool or uint8 tensor"):
        mesh.select(torch.zeros(2, dtype=torch.int64))
    with pytest.raises(ValueError, match=r"keep must be \[K\]"):
        mesh.select(torch.zeros(2, 1, dtype=torch.bool))
    with pytest.raises(ValueError, match="sequence of part ids"):
        mesh.select([0.5])
    with pytest.raises(ValueError, match="sequence of part ids"):
        mesh.select(3)
    with pytest.raises(ValueError, match="sequence of part ids"):
        mesh.select(["a"])
    with pytest.raises(ValueError, match="negative"):
        mesh.select([0, -1])
    # length and range: need K
    for bad in (torch.zeros(3, dtype=torch.bool), torch.zeros(1, dtype=torch.uint8), torch.zeros(0, dtype=torch.uint8)):
        with pytest.raises(ValueError, match="keep has %d entries for 2 parts" % bad.shape[0]):
            mesh.select(bad, parts=parts)
    with pytest.raises(ValueError, match=r"part id 2 is outside \[0, 2\)"):
        mesh.select([0, 2], parts=parts)
    with pytest.raises(ValueError, match="must not be negative"):
        mesh.largest(-1, parts=parts)
    with pytest.raises(ValueError, match="MeshParts of this mesh"):
        mesh.largest(1, parts=(parts.vertex_part, parts.face_part))
    other = geometry.Mesh(torch.zeros(7, 3), mesh.faces, None)
    with pytest.raises(ValueError, match="parts labels 6 vertices"):
        other.select([0], parts=parts)
    # a good keep passes the checks and the call gets as far as the device check
    for keep in ([1], (0, 1), [], torch.tensor([True, False]), torch.tensor([0, 1], dtype=torch.uint8), np.array([1])):
        with pytest.raises(RuntimeError, match="must live on the GPU"):
            mesh.select(keep, parts=parts)
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        mesh.parts()


def test_the_ops_check_their_inputs():
    f = torch.zeros(4, 3, dtype=torch.int32)
    with pytest.raises(TypeError, match="faces must be a tensor"):
        ops.mesh_parts([[0, 1, 2]], 3)
    with pytest.raises(ValueError, match=r"faces as \[n,3\]"):
        ops.mesh_parts(torch.zeros(4, 4, dtype=torch.int32), 3)
    with pytest.raises(TypeError, match="faces must be torch.int32"):
        ops.mesh_parts(torch.zeros(4, 3, dtype=torch.int64), 3)
    with pytest.raises(ValueError, match="n_vertices must lie in"):
        ops.mesh_parts(f, -1)
    with pytest.raises(ValueError, match="n_vertices must lie in"):
        ops.mesh_parts(f, 2 ** 31)
    with pytest.raises(RuntimeError, match="faces must live on the GPU"):
        ops.mesh_parts(f, 3)
    v, vp, fp, keep = torch.zeros(5, 3), torch.zeros(5, dtype=torch.int32), torch.zeros(4, dtype=torch.int32), torch.zeros(2, dtype=torch.uint8)
    with pytest.raises(ValueError, match=r"vertices as \[n,3\]"):
        ops.mesh_select(torch.zeros(5), f, None, vp, fp, keep)
    with pytest.raises(ValueError, match="normals must have 5 rows"):
        ops.mesh_select(v, f, torch.zeros(4, 3), vp, fp, keep)
    with pytest.raises(TypeError, match="keep must be a uint8 or bool tensor"):
        ops.mesh_select(v, f, None, vp, fp, torch.zeros(2))
    with pytest.raises(ValueError, match="more than the 5 vertices"):
        ops.mesh_select(v, f, None, vp, fp, torch.zeros(6, dtype=torch.uint8))
    with pytest.raises(ValueError, match="vertex_part must have 5 rows"):
        ops.mesh_select(v, f, None, fp, fp, keep)
    with pytest.raises(ValueError, match="face_part must have 4 rows"):
        ops.mesh_select(v, f, None, vp, vp, keep)
    with pytest.raises(TypeError, match="face_part must be torch.int32"):
        ops.mesh_select(v, f, None, vp, fp.long(), keep)
    with pytest.raises(RuntimeError, match="vertices must live on the GPU"):
        ops.mesh_select(v, f, None, vp, fp, keep)


# ---------------------------------------------------------------- the restatement itself
@pytest.mark.parametrize("name", sorted(C.HAND))
def test_the_restatement_on_hand_cases(name):
    f, V, vp, fp = C.hand(name)
    got = C.parts_ref(f, V)
    assert [a.dtype for a in got] == [np.int32] * 4
    assert np.array_equal(got[0], vp) and np.array_equal(got[1], fp), name
    K = int(vp.max()) + 1 if V else 0
    assert np.array_equal(got[2], np.bincount(vp, minlength=K)) and np.array_equal(got[3], np.bincount(fp[fp >= 0], minlength=K))
    # reversing the face order changes nothing but the order of face_part
    back = C.parts_ref(f[::-1], V)
    assert np.array_equal(back[0], vp) and np.array_equal(back[1], fp[::-1])


def test_the_restatement_selects_and_ranks_by_the_rules():
    f, V, vp, fp = C.hand("bad ids")
    v = np.arange(3 * V, dtype=np.float32).reshape(V, 3)
    sv, sf, sn = C.select_ref(v, f, None, vp, fp, [0, 1])
    assert sn is None and np.array_equal(sv, v[3:]) and np.array_equal(sf, [[0, 1, 2], [1, 2, 0]])      # the invalid faces are never selected
    sv, sf, sn = C.select_ref(v, f, -v, vp, fp, [1, 1])
    assert np.array_equal(sv, v) and np.array_equal(sn, -v) and np.array_equal(sf, f[[0, 2, 4]])
    f, V, vp, fp = C.hand("interleaved ids")
    sv, sf, _ = C.select_ref(v, f, None, vp, fp, [0, 1])
    assert np.array_equal(sv, v[[1, 3, 5]]) and np.array_equal(sf, [[0, 1, 2]])
    assert np.array_equal(sf, C.select_ref(v, f, None, vp, fp, np.array([False, True]))[1])
    # labels outside [0, K) count as not kept
    sv, sf, _ = C.select_ref(v, f, None, np.array([0, 7, 0, -2, 0, 1]), np.array([0, 9]), [1, 1])
    assert np.array_equal(sv, v[[0, 2, 4, 5]]) and np.array_equal(sf, [[0, 1, 2]])
    assert C.largest_ref([5, 9, 9, 1], 1).tolist() == [0, 1, 0, 0]
    assert C.largest_ref([5, 9, 9, 1], 2).tolist() == [0, 1, 1, 0]
    assert C.largest_ref([5, 9, 9, 1], 3).tolist() == [1, 1, 1, 0]
    assert C.largest_ref([5, 9, 9, 1], 9).tolist() == [1, 1, 1, 1]
    assert C.largest_ref([3, 3], 1).tolist() == [1, 0] and C.largest_ref([], 1).tolist() == [] and C.largest_ref([4], 0).tolist() == [0]


def _scipy_labels(faces, V):
    """scipy's components, relabelled by first vertex; None when scipy is not there."""
    try:
        from scipy.sparse import coo_matrix
        from scipy.sparse.csgraph import connected_components
    except ImportError:
        return None
    fv = np.asarray(faces, dtype=np.int64)[C.valid_faces(faces, V)]
    rows, cols = np.concatenate([fv[:, 0], fv[:, 0]]), np.concatenate([fv[:, 1], fv[:, 2]])
    k, lab = connected_components(coo_matrix((np.ones(len(rows)), (rows, cols)), shape=(V, V)), directed=False)
    first = np.full(k, V)
    np.minimum.at(first, lab, np.arange(V))
    return np.argsort(np.argsort(first))[lab]


def test_the_restatement_on_the_blobs_against_the_known_counts_and_scipy():
    v, f, n = C.mesh("blobs33")
    vp, fp, pv, pf = C.parts("blobs33")
    assert (len(v), len(f), len(pv)) == (4272, 8490, 6)
    assert pf.tolist() == [434, 5796, 632, 408, 1104, 116] and pv.sum() == len(v) and (fp >= 0).all()
    assert C.largest_ref(pf, 1).tolist() == [0, 1, 0, 0, 0, 0]
    chi = []
    for k in range(6):
        keep = np.arange(6) == k
        sv, sf, _ = C.select_ref(v, f, None, vp, fp, keep)
        assert (len(sv), len(sf)) == (pv[k], pf[k])
        t = M.topology(sf, len(sv))
        assert t["unused"] == 0 and t["directed_max"] == 1
        chi.append(t["chi"])
    assert chi == [1, 2, 2, 2, 2, 2]                   # part 0 is the blob the box cuts open; the others are closed
    # the cavity (part 2) lies inside the id range of the outer surface (part 1): kept and dropped rows interleave
    inner, outer = np.nonzero(vp == 2)[0], np.nonzero(vp == 1)[0]
    assert outer.min() < inner.min() and inner.max() < outer.max()
    assert len(C.parts("blobs17")[2]) == 5             # the smallest floater falls between the nodes
    ref = _scipy_labels(f, len(v))
    if ref is not None:
        assert np.array_equal(ref, vp)
        bad = f.copy()
        bad[5, 1], bad[77, 2] = -1, len(v)
        assert np.array_equal(_scipy_labels(bad, len(v)), C.parts_ref(bad, len(v))[0])


def test_the_restatement_on_the_tie_and_on_many_parts():
    vp, fp, pv, pf = C.parts("tie")
    assert pf.tolist() == [3456, 3456] and C.largest_ref(pf, 1).tolist() == [1, 0]
    v, f, _ = C.mesh("noise41-0.75")
    vp, fp, pv, pf = C.parts("noise41-0.75")
    assert (len(v), len(f), len(pv), int(pf.max())) == (102424, 189232, 2824, 1744)
    ref = _scipy_labels(f, len(v))
    if ref is not None:
        assert np.array_equal(ref, vp)

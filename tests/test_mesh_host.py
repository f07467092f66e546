"""Host-side checks of the mesh extraction (include/crnerf_mesh.h, crnerf_amd.geometry.Mesh; no GPU needed): the header against
its table of _lib.HEADER_SIGNATURES, the exports, every refusal of the entries -- each call below is refused, or is a no-op, on the host before any
device work, so the pointers are never followed --, the PLY writer on CPU tensors, the axis and threshold refusals of the geometry layer, and the
NumPy restatement the GPU tests compare with (tests/_mesh_cases.py) held to the topology a closed surface must have."""
import importlib.util
import os

import numpy as np
import pytest
import torch

from crnerf_amd import _lib, geometry, ops

import _abi
from _abi import bound as _fn, header_text as _header, last_error as _last_error
import _mesh_cases as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 4096          # a non-NULL, 16-byte aligned pointer that is never followed
BIG = 2 ** 31 - 1
COUNT, EMIT, BYTES = "crnerf_mesh_count_f32", "crnerf_mesh_emit_f32", "crnerf_mesh_workspace_bytes"
TABLE = _lib.HEADER_SIGNATURES["crnerf_mesh.h"]


def test_header_declares_the_three_entries_and_matches_the_signature_table():
    _abi.check_header("crnerf_mesh.h")                  # every return type and every parameter, by C type
    protos = _abi.prototypes("crnerf_mesh.h")
    assert list(protos) == list(TABLE) == [BYTES, COUNT, EMIT]
    assert len(protos[BYTES][1]) == 3 and len(protos[COUNT][1]) == 8 and len(protos[EMIT][1]) == 15
    # in no other header's table (tests/test_host.py: pairwise disjoint, 152 rows in all); the older headers do not know the entries
    assert not set(TABLE) & set().union(*(t for h, t in _lib.HEADER_SIGNATURES.items() if h != "crnerf_mesh.h"))
    assert "crnerf_mesh_" not in _header("crnerf.h") and "crnerf_mesh_" not in _header("crnerf_geometry.h")


def test_header_states_the_rules():
    text = _header("crnerf_mesh.h")
    for word in ("Inside.", "Edges.", "Vertices.", "Tetrahedra.", "Orientation.", "Rotation", "Face order.", "Degenerate", "Short axes.", "Normals.",
                 "xyz, xzy, yxz, yzx, zxy, zyx", "dx + 2 dy + 4 dz - 1", "t = 0.5"):
        assert word in text, word


def test_build_knows_the_unit_and_the_header():
    spec = importlib.util.spec_from_file_location("crnerf_build_for_mesh", os.path.join(ROOT, "cr-nerf-pytorch_amd", "build.py"))
    build = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(build)
    assert "mesh.hip" in build.SOURCES and all("../../include/" + header in build.HEADERS for header in _lib.HEADER_SIGNATURES)
    assert "-fhonor-nans" in build.PER_FILE_FLAGS["mesh.hip"]          # the inside test and the t fallback are NaN comparisons
    assert "-ffp-contract=off" in build.FLAGS                          # the interpolation: a multiply and an add


NEGATIVE = ((-1, 4, 4), (4, -1, 4), (4, 4, -1), (-1, 0, 4), (-2 ** 31, 2, 2))
TOO_MANY = ((2 ** 16, 2 ** 15, 1), (1, 2 ** 16, 2 ** 15), (1291, 1291, 1291), (BIG, 2, 1), (BIG, BIG, BIG), (46341, 46341, 1))
NOTHING = ((0, 4, 4), (4, 0, 4), (4, 4, 0), (0, 0, 0), (0, BIG, BIG), (1, 4, 4), (4, 1, 4), (4, 4, 1), (1, 1, 1), (BIG, 1, 1), (1, 1, BIG))
WORK = ((2, 2, 2), (4, 3, 2), (1290, 1290, 1290), (2, 2, (BIG - 1) // 4))


def test_count_refuses_before_any_device_work():
    fn = _fn(COUNT)
    for dims in NEGATIVE:
        assert fn(P, *dims, 0.0, P, P, None) == -2, dims                        # CRNERF_ERR_SHAPE
        assert _last_error() == b"mesh_count: negative axis length"
    for dims in TOO_MANY:
        assert fn(P, *dims, 0.0, P, P, None) == -2, dims
        assert _last_error().startswith(b"mesh_count: more than 2^31 - 1 nodes")
    for dims in NOTHING:                                                        # empty, or no cell: nothing to do, nothing is looked at
        assert fn(None, *dims, 0.0, None, None, None) == 0, dims                # (counts NULL: there is nowhere to write the two zeros)
        assert fn(P, *dims, 0.0, P, None, None) == 0, dims
    for k, field in enumerate((b"sigma", b"workspace", b"counts")):
        for dims in WORK:
            a = [P, P, P]
            a[k] = None
            assert fn(a[0], *dims, 0.0, a[1], a[2], None) == -1, (field, dims)  # CRNERF_ERR_NULL
            assert _last_error() == field + b" is NULL"
    assert fn(P, 2, 2, 2, 0.0, P + 8, P, None) == -3                            # CRNERF_ERR_CONFIG
    assert _last_error() == b"mesh_count: workspace must be 16-byte aligned"


def test_emit_refuses_before_any_device_work():
    fn = _fn(EMIT)

    def call(dims, v_cap=8, f_cap=8, sigma=P, xs=P, ys=P, zs=P, ws=P, v=P, n=P, f=P):
        return fn(sigma, xs, ys, zs, *dims, 0.0, ws, v_cap, f_cap, v, n, f, None)
    for dims in NEGATIVE:
        assert call(dims) == -2, dims
        assert _last_error() == b"mesh_emit: negative axis length"
    for dims in TOO_MANY:
        assert call(dims) == -2, dims
        assert _last_error().startswith(b"mesh_emit: more than 2^31 - 1 nodes")
    for caps in ((2 ** 31, 8), (8, 2 ** 31), (2 ** 40, 2 ** 40), (2 ** 63 - 1, 0)):
        for dims in WORK + NOTHING[:3]:
            assert call(dims, *caps) == -2, (caps, dims)
            assert _last_error().startswith(b"mesh_emit: a capacity above 2^31 - 1")
    for caps in ((-1, 8), (8, -1)):
        assert call((4, 4, 4), *caps) == -2
        assert _last_error() == b"mesh_emit: negative capacity"
    for dims in NOTHING:
        assert call(dims, sigma=None, xs=None, ys=None, zs=None, ws=None, v=None, n=None, f=None) == 0, dims
        assert call(dims, BIG, BIG) == 0, dims
    assert call((4, 4, 4), 0, 0, sigma=None, xs=None, ys=None, zs=None, ws=None, v=None, n=None, f=None) == 0      # room for nothing
    for field in ("sigma", "xs", "ys", "zs", "ws", "v", "f"):
        for dims in WORK:
            for caps in ((8, 8), (BIG, BIG)):
                assert call(dims, *caps, **{field: None}) == -1, (field, dims)
                assert _last_error() == {"ws": b"workspace", "v": b"vertices", "f": b"faces"}.get(field, field.encode()) + b" is NULL"
    assert call((4, 4, 4), 0, 8, v=None, ws=None) == -1 and _last_error() == b"workspace is NULL"      # vertices may be NULL when v_cap == 0 ...
    assert call((4, 4, 4), 8, 0, f=None, ws=None) == -1 and _last_error() == b"workspace is NULL"      # ... faces when f_cap == 0
    assert call((4, 4, 4), ws=P + 2) == -3
    assert _last_error() == b"mesh_emit: workspace must be 16-byte aligned"


def test_workspace_bytes_is_monotone_and_zero_for_an_empty_grid():
    fn = _fn(BYTES)
    for dims in ((0, 4, 4), (4, 0, 4), (4, 4, 0), (0, 0, 0), (-1, 4, 4), (4, 4, -7)) + TOO_MANY:
        assert fn(*dims) == 0, dims
    assert fn(1, 1, 1) > 0
    for base in ((1, 1, 1), (2, 2, 2), (31, 33, 32), (1024, 1, 1), (300, 200, 100)):
        for axis in range(3):
            prev = fn(*base)
            for step in (1, 2, 7, 1000):
                dims = list(base)
                dims[axis] += step
                now = fn(*dims)
                assert now > prev, (base, axis, step)
                prev = now
    n = 1290 ** 3
    assert fn(1290, 1290, 1290) >= 5 * n                # the masks and the two 16-bit offsets of every node
    assert fn(BIG, 1, 1) >= 5 * BIG


# ---------------------------------------------------------------- the Python layer
def _ply(path):
    """A minimal reader of what save_ply writes: (vertex rows [V, 3 or 6] float32, faces [F,3] int32, property names)."""
    with open(path, "rb") as f:
        blob = f.read()
    end = blob.index(b"end_header\n") + len(b"end_header\n")
    lines = blob[:end].decode("ascii").split("\n")
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0"
    V = int([ln for ln in lines if ln.startswith("element vertex")][0].split()[2])
    F = int([ln for ln in lines if ln.startswith("element face")][0].split()[2])
    props = [ln.split()[2] for ln in lines if ln.startswith("property float ")]
    assert "property list uchar int vertex_indices" in lines
    assert lines.index("element vertex %d" % V) < lines.index("property float x") < lines.index("element face %d" % F)
    v = np.frombuffer(blob, dtype="<f4", count=V * len(props), offset=end).reshape(V, len(props))
    rows = np.frombuffer(blob, dtype=np.dtype([("n", "u1"), ("i", "<i4", (3,))]), count=F, offset=end + 4 * V * len(props))
    assert end + 4 * V * len(props) + 13 * F == len(blob)
    assert (rows["n"] == 3).all()
    return v, rows["i"], props


@pytest.mark.parametrize("with_normals", [True, False])
def test_save_ply_round_trip_on_cpu_tensors(tmp_path, with_normals):
    s, xs, ys, zs = M.sphere(9)
    v, f, n = M.mesh_ref(s, xs, ys, zs, 0.0)
    mesh = geometry.Mesh(torch.from_numpy(v), torch.from_numpy(f), torch.from_numpy(n.astype(np.float32)) if with_normals else None)
    path = str(tmp_path / "m.ply")
    mesh.save_ply(path)
    rows, faces, props = _ply(path)
    assert props == (["x", "y", "z", "nx", "ny", "nz"] if with_normals else ["x", "y", "z"])
    assert np.array_equal(rows[:, :3], v) and np.array_equal(faces, f)
    if with_normals:
        assert np.array_equal(rows[:, 3:], n.astype(np.float32))
    empty = geometry.Mesh(torch.zeros(0, 3), torch.zeros(0, 3, dtype=torch.int32), None)
    empty.save_ply(path)
    rows, faces, props = _ply(path)
    assert rows.shape == (0, 3) and faces.shape == (0, 3)


def test_geometry_layer_refuses_axes_that_do_not_rise_and_a_nan_threshold():
    up = torch.linspace(-1.0, 1.0, 4)
    sigma = torch.zeros(4, 4, 4)
    for k in range(3):
        for bad in (torch.tensor([1.0, 0.5, 0.0, -1.0]), torch.tensor([0.0, 0.5, 0.5, 1.0]), torch.tensor([0.0, float("nan"), 0.5, 1.0]),
                    torch.tensor([0.0, 1.0, 0.5, 2.0])):
            axes = [up, up, up]
            axes[k] = bad
            with pytest.raises(ValueError, match="axis %s is not strictly increasing" % ("xs", "ys", "zs")[k]):
                geometry.DensityGrid(sigma, *axes).mesh(0.0)
    with pytest.raises(ValueError, match="threshold is NaN"):
        geometry.DensityGrid(sigma, up, up, up).mesh(float("nan"))
    with pytest.raises(ValueError, match="threshold is NaN"):
        geometry.extract_mesh(None, (-1, -1, -1), (1, 1, 1), 4, float("nan"))
    # rising axes pass the check and the call gets as far as the device check
    with pytest.raises(RuntimeError, match="sigma must live on the GPU"):
        geometry.DensityGrid(sigma, up, up, up).mesh(0.0)


def test_mesh_grid_checks_its_inputs_like_the_density_query():
    up = torch.linspace(-1.0, 1.0, 4)
    with pytest.raises(TypeError, match="sigma must be a tensor"):
        ops.mesh_grid([[0.0]], up, up, up, 0.0)
    with pytest.raises(ValueError, match=r"sigma as \[nz, ny, nx\]"):
        ops.mesh_grid(torch.zeros(4, 4), up, up, up, 0.0)
    with pytest.raises(ValueError, match=r"the axis ys as \[n\]"):
        ops.mesh_grid(torch.zeros(4, 4, 4), up, torch.zeros(4, 1), up, 0.0)
    with pytest.raises(ValueError, match=r"sigma must be \[nz, ny, nx\] = \(3, 4, 5\)"):
        ops.mesh_grid(torch.zeros(5, 4, 3), torch.zeros(5), torch.zeros(4), torch.zeros(3), 0.0)
    with pytest.raises(RuntimeError, match="sigma must live on the GPU"):
        ops.mesh_grid(torch.zeros(4, 4, 4), up, up, up, 0.0)


# ---------------------------------------------------------------- the restatement itself
def test_the_restatement_gives_closed_oriented_surfaces():
    s, xs, ys, zs = M.sphere(17)
    v, f, n = M.mesh_ref(s, xs, ys, zs, 0.0)
    assert v.dtype == np.float32 and f.dtype == np.int32 and n.dtype == np.float64
    assert (len(v), len(f)) == (1730, 3456)
    t = M.topology(f, len(v))
    assert t["uses"] == {2: t["E"]} and t["directed_max"] == 1 and t["chi"] == 2 and t["unused"] == 0
    centres = v[f].astype(np.float64).mean(1)
    assert (np.einsum("ij,ij->i", M.face_normals(v, f), centres) > 0).all()          # every face looks away from the centre
    unit = v / np.linalg.norm(v, axis=1, keepdims=True)
    assert np.einsum("ij,ij->i", n, unit).min() > 0.999                               # and so does every normal
    # a shared vertex is one vertex: (node, direction) order means the ids rise with the owning node
    s, xs, ys, zs = M.torus(17)
    v, f, _ = M.mesh_ref(s, xs, ys, zs, 0.0)
    t = M.topology(f, len(v))
    assert t["uses"] == {2: t["E"]} and t["directed_max"] == 1 and t["chi"] == 0 and t["unused"] == 0
    # rotation: the first id of every face is its smallest
    assert (f[:, 0] == f.min(axis=1)).all()
    assert M.mesh_ref(s[:1], xs, ys, zs[:1], 0.0)[0].shape == (0, 3)

"""Host-side checks of the mesh simplification (csrc/crnerf_mesh_simplify.h, staged beside the sources; ops.mesh_cluster; crnerf_amd.geometry
Mesh.simplify / extract_mesh(simplify_cell=); no GPU needed): the staged header against _lib.STAGED_MESH_SIGNATURES parameter by parameter, the
exports and where they are bound, every refusal and no-op of the entries -- each call below is refused, or does nothing, on the host before any
device work, so the pointers are never followed --, the refusals of the Python layer that fire before a device tensor is needed, and the NumPy
restatement the GPU tests compare with (tests/_mesh_simplify_cases.py) held to hand cases small enough to check by eye."""
import ctypes
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

import _abi
from _abi import last_error as _last_error
from crnerf_amd import _lib, geometry, ops

import _mesh_simplify_cases as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cr-nerf-pytorch_amd", "csrc")
HEADER = "crnerf_mesh_simplify.h"
BYTES, COUNT, EMIT = "crnerf_mesh_cluster_workspace_bytes", "crnerf_mesh_cluster_count_f32", "crnerf_mesh_cluster_emit_f32"
ENTRIES = [BYTES, COUNT, EMIT]
P = 4096          # a non-NULL, 16-byte aligned pointer that is never followed
BIG = 2 ** 31 - 1
SHAPE, NULL, CONFIG = -2, -1, -3          # CRNERF_ERR_*
GRID = (0.0, 0.0, 0.0, 1.0, 1.0, 1.0, 2, 2, 2)
INF, NAN = float("inf"), float("nan")


def _fn(name):
    """Entry `name` of the built library on a handle of its own, bound as the staged table says."""
    assert os.path.exists(_lib.LIB_PATH), "libcrnerf_hip.so missing: run __graft_entry__.build()"
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, name), "%s is not exported" % name
    fn = getattr(lib, name)
    fn.restype, fn.argtypes = _lib.STAGED_MESH_SIGNATURES[HEADER][name]
    return fn


# ---------------------------------------------------------------- the header, the table, the binding
def test_staged_header_matches_the_staged_mesh_table_parameter_by_parameter(monkeypatch):
    monkeypatch.setattr(_abi, "INCLUDE", CSRC)
    assert list(_lib.STAGED_MESH_SIGNATURES) == [HEADER] and os.path.exists(os.path.join(CSRC, HEADER))
    protos, table = _abi.prototypes(HEADER), _lib.STAGED_MESH_SIGNATURES[HEADER]
    assert list(protos) == list(table) == ENTRIES
    text = re.sub(r"/\*.*?\*/", "", _abi.header_text(HEADER), flags=re.S)
    assert sorted(set(re.findall(r"\b(crnerf_[a-z0-9_]+)\s*\(", text))) == sorted(table)      # nothing that looks like an entry escaped the parser
    assert "struct" not in text                                                                 # the grid is nine scalars
    for symbol, (ret, params) in protos.items():
        restype, argtypes = table[symbol]
        assert restype is _abi.RESTYPES[ret], symbol
        assert len(argtypes) == len(params), symbol
        for k, (decl, argtype) in enumerate(zip(params, argtypes)):
            assert argtype is _abi.expected_argtype(symbol, decl), "%s, parameter %d (%s): the table says %s" % (symbol, k, decl, argtype)
    assert [protos[n][0] for n in ENTRIES] == ["size_t", "int", "int"] and [len(protos[n][1]) for n in ENTRIES] == [3, 17, 24]
    grid = ["lo0", "lo1", "lo2", "cell0", "cell1", "cell2", "n0", "n1", "n2"]
    names = {n: [d.split()[-1].lstrip("*") for d in protos[n][1]] for n in ENTRIES}
    assert names[BYTES] == ["V", "F", "cells"]
    assert names[COUNT] == ["vertices", "faces", "V", "F"] + grid + ["workspace", "vertex_cluster", "counts", "stream"]
    assert names[EMIT] == (["vertices", "normals", "colors", "faces", "vertex_cluster", "V", "F"] + grid
                           + ["workspace", "v_cap", "f_cap", "out_vertices", "out_normals", "out_colors", "out_faces", "stream"])
    for n in (COUNT, EMIT):                                                                     # no host pointer: the nine are float / int32_t by value
        at = names[n].index("lo0")
        assert [" ".join(d.split()[:-1]) for d in protos[n][1][at:at + 9]] == ["float"] * 6 + ["int32_t"] * 3


def test_header_states_the_rules():
    with open(os.path.join(CSRC, HEADER)) as f:
        text = f.read()
    first = text.split("*/")[0]
    assert "STAGED" in first and "include/" in first and "tests/test_host.py" in first and "STAGED_MESH_SIGNATURES" in first
    for word in ("Arithmetic.", "-ffp-contract=off", "Domain.", "-fno-honor-nans", "Cell of a vertex.", "Clusters.", "Cluster position.",
                 "Cluster normal", "Cluster colour", "Faces.", "Unused clusters.", "never dereferenced", "smallest member vertex id",
                 "1048576.0f", "exact in float32", "not a byte copy", "smallest input index", "smallest id comes first", "drop_small(1)",
                 "same bytes on every run", "function of the input alone", "nine"):
        assert word in text, word


def test_entries_are_exported_bound_and_outside_the_other_tables():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    bound = _lib.load()
    for name in ENTRIES:
        assert hasattr(lib, name), name
        assert name not in _lib.ALL_SIGNATURES and name not in _lib.EXPORTS, name
        assert all(name not in table for table in _lib.HEADER_SIGNATURES.values())
        assert all(name not in table for table in _lib.STAGED_SIGNATURES.values())
        fn = getattr(bound, name)
        res, args = _lib.STAGED_MESH_SIGNATURES[HEADER][name]
        assert fn.restype is res and list(fn.argtypes) == args, name
    assert HEADER not in _lib.HEADER_SIGNATURES and HEADER not in _lib.STAGED_SIGNATURES
    assert HEADER not in os.listdir(os.path.join(ROOT, "include"))
    assert _lib.STAGED_MAPPINGS == (_lib.STAGED_SIGNATURES, _lib.STAGED_MESH_SIGNATURES)


def test_load_names_a_missing_symbol_of_the_second_mapping(monkeypatch):
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setitem(_lib.STAGED_MESH_SIGNATURES, "crnerf_not_there.h", {"crnerf_mesh_not_there_f32": (ctypes.c_int, [])})
    with pytest.raises(AttributeError, match="does not export crnerf_mesh_not_there_f32, which csrc/crnerf_not_there.h declares"):
        _lib.load()
    assert _lib._lib is None      # nothing half-bound is kept (monkeypatch puts the loaded handle back)


def test_the_duplicate_check_at_import_covers_both_mappings():
    with open(os.path.join(ROOT, "cr-nerf-pytorch_amd", "_lib.py")) as f:
        source = f.read()
    # a copy of the module in which the second mapping declares an entry of the first: the import must refuse it
    twice = source.replace('"crnerf_mesh_cluster_workspace_bytes": (usz, [i64, i64, i64]),',
                           '"crnerf_mesh_cluster_workspace_bytes": (usz, [i64, i64, i64]), "crnerf_feature_points_f32": (i32, []),')
    assert twice != source
    with pytest.raises(ImportError, match="crnerf_feature_points_f32"):
        exec(compile(twice, "_lib_twice.py", "exec"), {"__name__": "crnerf_lib_twice", "__file__": _lib.__file__})
    counted = source.replace('"crnerf_mesh_cluster_workspace_bytes": (usz, [i64, i64, i64]),',
                             '"crnerf_mesh_cluster_workspace_bytes": (usz, [i64, i64, i64]), "crnerf_mesh_count_f32": (i32, []),')
    with pytest.raises(ImportError, match="crnerf_mesh_count_f32"):
        exec(compile(counted, "_lib_counted.py", "exec"), {"__name__": "crnerf_lib_counted", "__file__": _lib.__file__})


def test_build_knows_the_unit_and_the_header():
    spec = importlib.util.spec_from_file_location("crnerf_build_for_mesh_simplify", os.path.join(ROOT, "cr-nerf-pytorch_amd", "build.py"))
    build = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(build)
    assert "mesh_simplify.hip" in build.SOURCES and os.path.exists(os.path.join(CSRC, "mesh_simplify.hip"))
    assert HEADER in build.HEADERS      # an edit of the staged header rebuilds
    assert "mesh_simplify.hip" not in build.PER_FILE_FLAGS and "-ffp-contract=off" in build.FLAGS and "-ffast-math" not in build.FLAGS


# ---------------------------------------------------------------- refusals and no-ops of the entries
NEGATIVE = ((-1, 4), (4, -1), (-1, -1), (-2 ** 63, 0))
TOO_MANY = ((2 ** 31, 4), (4, 2 ** 31), (2 ** 40, 2 ** 40), (2 ** 63 - 1, 1))
WORK = ((1, 0), (5, 0), (3, 1), (BIG, BIG), (4, BIG))
BAD_GRIDS = [((0, 0, 0, 1, 1, 1, 0, 2, 2), b"fewer than one cell on an axis"), ((0, 0, 0, 1, 1, 1, 2, -3, 2), b"fewer than one cell on an axis"),
             ((0, 0, 0, 1, 1, 1, 2, 2, 2 ** 20 + 1), b"more than 2^20 cells on an axis"), ((0, 0, 0, 1, 1, 1, 2 ** 31 - 1, 1, 1), b"more than 2^20 cells on an axis"),
             ((0, 0, 0, 1, 1, 1, 2 ** 11, 2 ** 10, 2 ** 10), b"more than 2^31 - 1 cells"), ((0, 0, 0, 1, 1, 1, 2 ** 20, 2 ** 20, 2 ** 20), b"more than 2^31 - 1 cells"),
             ((0, 0, 0, 0.0, 1, 1, 2, 2, 2), b"a cell size that is not finite and > 0"), ((0, 0, 0, 1, -1.0, 1, 2, 2, 2), b"a cell size that is not finite and > 0"),
             ((0, 0, 0, 1, 1, INF, 2, 2, 2), b"a cell size that is not finite and > 0"), ((0, 0, 0, NAN, 1, 1, 2, 2, 2), b"a cell size that is not finite and > 0"),
             ((0, 0, 0, 1, 1e-45, 1, 2, 2, 2), b"a cell size whose float32 reciprocal is not finite"),
             ((INF, 0, 0, 1, 1, 1, 2, 2, 2), b"a box origin that is not finite"), ((0, -INF, 0, 1, 1, 1, 2, 2, 2), b"a box origin that is not finite"),
             ((0, 0, NAN, 1, 1, 1, 2, 2, 2), b"a box origin that is not finite")]
GOOD_GRIDS = [GRID, (-1.0, -1.0, -1.0, 2 / 128, 2 / 128, 2 / 128, 128, 128, 128), (0, 0, 0, 1e-30, 1e30, 1, 2 ** 20, 2 ** 10, 1), (5, 5, 5, 3, 3, 3, 1, 1, 1),
              (0, 0, 0, 1, 1, 1, 2 ** 11 - 1, 2 ** 10, 2 ** 10)]


def test_count_refuses_before_any_device_work():
    fn = _fn(COUNT)
    who = b"mesh_cluster_count: "
    for V, F in NEGATIVE:
        assert fn(P, P, V, F, *GRID, P, P, P, None) == SHAPE, (V, F)
        assert _last_error() == who + b"negative size"
    for V, F in TOO_MANY:
        assert fn(P, P, V, F, *GRID, P, P, P, None) == SHAPE, (V, F)
        assert _last_error().startswith(who + b"more than 2^31 - 1")
    for grid, text in BAD_GRIDS:
        for V, F in ((4, 4), (0, 0), (BIG, BIG)):                    # the grid is judged even when there is no vertex
            assert fn(P, P, V, F, *grid, P, P, P, None) == SHAPE, grid
            assert _last_error() == who + text, grid
    for grid in GOOD_GRIDS:
        for F in (0, 7, BIG):                                       # no vertex: nothing to do, nothing is looked at (counts NULL: nowhere to write the zeros)
            assert fn(None, None, 0, F, *grid, None, None, None, None) == 0
            assert fn(P, P, 0, F, *grid, P + 8, P, None, None) == 0
    for V, F in WORK:
        for k, field in ((0, b"vertices"), (1, b"faces"), (13, b"workspace"), (14, b"vertex_cluster"), (15, b"counts")):
            a = [P, P, V, F, *GRID, P, P, P, None]
            a[k] = None
            if F == 0 and field == b"faces":                         # no face: not needed; the call gets as far as the alignment check
                a[13] = P + 8
                assert fn(*a) == CONFIG, (field, V, F)
                continue
            assert fn(*a) == NULL, (field, V, F)
            assert _last_error() == who + field + b" is NULL"
        assert fn(P, P, V, F, *GRID, P + 8, P, P, None) == CONFIG
        assert _last_error() == who + b"workspace must be 16-byte aligned"


def test_emit_refuses_before_any_device_work():
    fn = _fn(EMIT)
    who = b"mesh_cluster_emit: "

    def call(V=4, F=4, v_cap=8, f_cap=8, grid=GRID, vertices=P, normals=P, colors=P, faces=P, vertex_cluster=P, workspace=P, out_vertices=P,
             out_normals=P, out_colors=P, out_faces=P):
        return fn(vertices, normals, colors, faces, vertex_cluster, V, F, *grid, workspace, v_cap, f_cap, out_vertices, out_normals, out_colors,
                  out_faces, None)
    for V, F in NEGATIVE:
        assert call(V, F) == SHAPE and _last_error() == who + b"negative size"
    for V, F in TOO_MANY:
        assert call(V, F) == SHAPE and _last_error().startswith(who + b"more than 2^31 - 1")
    for caps in ((2 ** 31, 8), (8, 2 ** 31), (2 ** 40, 2 ** 40), (2 ** 63 - 1, 0)):
        assert call(BIG, BIG, *caps) == SHAPE and _last_error().startswith(who + b"a capacity above 2^31 - 1")
    for caps in ((-1, 8), (8, -1)):
        assert call(4, 4, *caps) == SHAPE and _last_error() == who + b"negative capacity"
    for grid, text in BAD_GRIDS:
        assert call(grid=grid) == SHAPE and _last_error() == who + text, grid
        assert call(0, 0, 0, 0, grid=grid) == SHAPE
    nothing = dict(vertices=None, normals=None, colors=None, faces=None, vertex_cluster=None, workspace=None, out_vertices=None, out_normals=None,
                   out_colors=None, out_faces=None)
    assert call(0, 0, **nothing) == 0 and call(0, 9, BIG, BIG, **nothing) == 0          # no vertex
    assert call(9, 9, 0, 0, **nothing) == 0                                              # room for nothing
    assert call(9, 0, 0, 8, **nothing) == 0                                              # room for faces only, and there are none
    for field in ("vertices", "faces", "vertex_cluster", "workspace", "out_vertices", "out_normals", "out_colors", "out_faces"):
        for V, F in ((4, 4), (BIG, BIG)):
            assert call(V, F, BIG, BIG, **{field: None}) == NULL, field
            assert _last_error() == who + field.encode() + b" is NULL"
    assert call(normals=None, out_normals=None, workspace=P + 8) == CONFIG               # no normals: out_normals is not needed
    assert call(colors=None, out_colors=None, workspace=P + 8) == CONFIG                 # no colours: out_colors is not needed
    assert call(v_cap=0, vertices=None, normals=None, colors=None, out_vertices=None, out_normals=None, out_colors=None, workspace=P + 8) == CONFIG      # faces only
    assert call(f_cap=0, faces=None, out_faces=None, workspace=P + 8) == CONFIG          # vertices only
    assert call(F=0, faces=None, out_faces=None, workspace=P + 8) == CONFIG
    assert _last_error() == who + b"workspace must be 16-byte aligned"


def test_workspace_bytes_is_monotone_and_zero_for_what_the_calls_refuse():
    fn = _fn(BYTES)
    for V, F in ((0, 0), (0, 9), (-1, 4), (4, -1)) + TOO_MANY:
        assert fn(V, F, 8) == 0, (V, F)
    for cells in (0, -1, 2 ** 31, 2 ** 62):
        assert fn(4, 4, cells) == 0, cells
    assert fn(1, 0, 1) > 0
    for V, F, cells in ((1, 0, 1), (5, 7, 8), (1024, 1024, 4096), (4272, 8490, 16 ** 3)):
        for step in (1, 2, 7, 1000):
            assert fn(V + step, F, cells) > fn(V, F, cells) and fn(V, F + step, cells) >= fn(V, F, cells) + 18 * step
            assert fn(V, F, cells + step) >= fn(V, F, cells) + 4 * step
    # the table: the smallest power of two >= 2 F slots of four bytes; the sums: 84 bytes for each of min(V, cells) clusters
    assert fn(10, 1025, 8) - fn(10, 1024, 8) >= 4 * 2048 and fn(10, 1024, 8) - fn(10, 1023, 8) < 64
    assert fn(100, 0, 8) - fn(99, 0, 8) < 32 and fn(8, 0, 100) - fn(7, 0, 100) >= 84
    assert fn(BIG, BIG, BIG) >= 4 * BIG + 6 * BIG + 18 * BIG + 4 * 2 ** 32 + 84 * BIG


# ---------------------------------------------------------------- the Python layer
V4 = torch.tensor([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [1.0, 1.0, 1.0]])      # on the CPU
F2 = torch.tensor([[0, 1, 2], [1, 3, 2]], dtype=torch.int32)


def test_simplify_refuses_a_bad_cell_or_box_before_any_device_work():
    mesh = geometry.Mesh(V4, F2)
    for bad in (0.0, -1.0, INF, NAN, (1.0, 0.0, 1.0), (1.0, 1.0, NAN), (1.0, 2.0), (1.0, 2.0, 3.0, 4.0), "a", None, [[1.0], [1.0], [1.0]]):
        with pytest.raises(ValueError, match="simplify: cell must be"):
            mesh.simplify(bad)
        with pytest.raises(ValueError, match="simplify: cell must be"):
            mesh.simplify(bad, lo=(0, 0, 0), hi=(1, 1, 1))
    with pytest.raises(ValueError, match="simplify: lo must be"):
        mesh.simplify(0.5, lo=(0, 0), hi=(1, 1, 1))
    with pytest.raises(ValueError, match="simplify: lo must be"):
        mesh.simplify(0.5, lo=(0, NAN, 0), hi=(1, 1, 1))
    with pytest.raises(ValueError, match="simplify: hi must be"):
        mesh.simplify(0.5, lo=(0, 0, 0), hi=(1, INF, 1))
    with pytest.raises(ValueError, match="simplify: hi must be"):
        mesh.simplify(0.5, hi=1.0)
    with pytest.raises(ValueError, match="simplify: hi must not lie below lo"):
        mesh.simplify(0.5, lo=(0, 0, 0), hi=(1, -1, 1))
    with pytest.raises(ValueError, match=r"simplify: cell = .* more than 2\^20 cells on an axis"):
        mesh.simplify(1e-7, lo=(0, 0, 0), hi=(1, 1, 1))
    with pytest.raises(ValueError, match=r"simplify: cell = .* more than 2\^20 cells on an axis"):
        mesh.simplify((1.0, 1.0, 1e-320), lo=(0, 0, 0), hi=(1, 1, 1e300))
    with pytest.raises(ValueError, match=r"simplify: cell = .*2048 x 1024 x 1024 cells, more than 2\^31 - 1 in all"):
        mesh.simplify(1.0, lo=(0, 0, 0), hi=(2048, 1024, 1024))
    # a good call passes the checks and gets as far as the device check; 2047 x 1024 x 1024 cells fit
    for kw in (dict(), dict(lo=(0, 0, 0), hi=(1, 1, 1)), dict(lo=(0, 0, 0)), dict(hi=(2047, 1024, 1024), lo=(0, 0, 0))):
        with pytest.raises(RuntimeError, match="vertices must live on the GPU"):
            mesh.simplify(1.0, **kw)
    with pytest.raises(RuntimeError, match="vertices must live on the GPU"):
        geometry.Mesh(V4, F2, V4, V4).simplify((0.5, 0.25, 1.0))


def test_simplify_of_an_empty_mesh_is_an_empty_mesh_without_a_device():
    e3, f0 = torch.zeros(0, 3), torch.zeros(0, 3, dtype=torch.int32)
    for mesh in (geometry.Mesh(e3, f0), geometry.Mesh(e3, F2), geometry.Mesh(e3, f0, e3), geometry.Mesh(e3, f0, e3, e3), geometry.Mesh(e3, f0, None, e3)):
        got = mesh.simplify(0.5)
        assert isinstance(got, geometry.Mesh) and got.vertices.shape == (0, 3) and got.faces.shape == (0, 3)
        assert got.vertices.dtype == torch.float32 and got.faces.dtype == torch.int32
        assert (got.normals is None) == (mesh.normals is None) and (got.colors is None) == (mesh.colors is None)
        for t in (got.normals, got.colors):
            assert t is None or t.shape == (0, 3)
    with pytest.raises(ValueError, match="cell must be"):
        geometry.Mesh(e3, f0).simplify(0.0)


class _Model:
    """Stands where a NeRF_sigma would: no refusal below gets as far as asking it for a pack."""
    def packed_weights(self, precision="f32"):
        raise AssertionError("the call should have been refused before the pack was asked for")


def test_extract_mesh_refuses_a_bad_simplify_cell_before_the_grid_is_paid_for():
    for bad in (0.0, -2.0, NAN, (1.0, 1.0)):
        with pytest.raises(ValueError, match="simplify: cell must be"):
            geometry.extract_mesh(_Model(), (-1, -1, -1), (1, 1, 1), 9, 0.5, simplify_cell=bad)
    with pytest.raises(AssertionError, match="before the pack"):      # a good cell: the call goes on to the model
        geometry.extract_mesh(_Model(), (-1, -1, -1), (1, 1, 1), 9, 0.5, simplify_cell=0.25)


def test_mesh_cluster_checks_its_inputs():
    v, f = V4, F2
    lo, cell, n = (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (2, 2, 2)
    with pytest.raises(TypeError, match="vertices must be a tensor"):
        ops.mesh_cluster(v.tolist(), f, lo, cell, n)
    with pytest.raises(ValueError, match=r"vertices as \[n,3\]"):
        ops.mesh_cluster(torch.zeros(4), f, lo, cell, n)
    with pytest.raises(TypeError, match="vertices must be torch.float32"):
        ops.mesh_cluster(v.double(), f, lo, cell, n)
    with pytest.raises(ValueError, match=r"faces as \[n,3\]"):
        ops.mesh_cluster(v, torch.zeros(2, 4, dtype=torch.int32), lo, cell, n)
    with pytest.raises(TypeError, match="faces must be torch.int32"):
        ops.mesh_cluster(v, f.long(), lo, cell, n)
    with pytest.raises(ValueError, match="normals must have 4 rows"):
        ops.mesh_cluster(v, f, lo, cell, n, normals=torch.zeros(3, 3))
    with pytest.raises(ValueError, match="colors must have 4 rows"):
        ops.mesh_cluster(v, f, lo, cell, n, colors=torch.zeros(5, 3))
    with pytest.raises(TypeError, match="colors must be torch.float32"):
        ops.mesh_cluster(v, f, lo, cell, n, colors=torch.zeros(4, 3, dtype=torch.uint8))
    for bad in (dict(lo=(0.0, 0.0)), dict(cell=1.0), dict(n=(2, 2)), dict(n=(2, 2, 2.5)), dict(lo="abc")):
        with pytest.raises(ValueError, match="3-sequences"):
            ops.mesh_cluster(v, f, **dict(dict(lo=lo, cell=cell, n=n), **bad))
    for bad in ((1.0, 0.0, 1.0), (1.0, -1.0, 1.0), (INF, 1.0, 1.0), (1.0, 1.0, NAN), (1e-45, 1.0, 1.0), (1e39, 1.0, 1.0)):
        with pytest.raises(ValueError, match="cell must be finite and > 0 as float32"):
            ops.mesh_cluster(v, f, lo, bad, n)
    for bad in ((INF, 0.0, 0.0), (0.0, NAN, 0.0), (0.0, 0.0, -1e39)):
        with pytest.raises(ValueError, match="lo must be finite as float32"):
            ops.mesh_cluster(v, f, bad, cell, n)
    for bad in ((0, 2, 2), (2, 2 ** 20 + 1, 2), (-1, 2, 2)):
        with pytest.raises(ValueError, match=r"1 to 2\^20 cells on every axis"):
            ops.mesh_cluster(v, f, lo, cell, bad)
    with pytest.raises(ValueError, match=r"more than 2\^31 - 1 cells"):
        ops.mesh_cluster(v, f, lo, cell, (2 ** 11, 2 ** 10, 2 ** 10))
    with pytest.raises(RuntimeError, match="vertices must live on the GPU"):
        ops.mesh_cluster(v, f, lo, cell, n, normals=v, colors=v)


# ---------------------------------------------------------------- the restatement itself
@pytest.mark.parametrize("name", sorted(S.HAND))
def test_the_restatement_on_hand_cases(name):
    case = S.hand(name)
    v, f = case["v"], case["f"]
    rng = np.random.default_rng(len(v))
    nrm = rng.standard_normal((len(v), 3)).astype(np.float32)
    nrm /= np.maximum(np.linalg.norm(nrm, axis=1, keepdims=True), 1e-9).astype(np.float32)
    col = rng.uniform(0, 1, (len(v), 3)).astype(np.float32)
    out_v, out_f, out_n, out_c, vc = S.cluster_ref(v, f, case["lo"], case["cell"], case["n"], nrm, col)
    assert (out_v.dtype, out_f.dtype, out_n.dtype, out_c.dtype, vc.dtype) == (np.float32, np.int32, np.float32, np.float32, np.int32)
    assert np.array_equal(vc, case["vc"]) and np.array_equal(out_f, case["out_f"]), name
    K = int(vc.max()) + 1 if len(vc) else 0
    assert out_v.shape == out_n.shape == out_c.shape == (K, 3) and out_f.shape[1:] == (3,)
    if "out_v" in case:
        assert np.array_equal(out_v, np.asarray(case["out_v"], np.float32)), (name, out_v)
    # every cluster lies in its cell, its colour between its members', its normal of unit length
    s, c, key = S.cells_ref(v, case["lo"], case["cell"], case["n"])
    lo, cell = np.asarray(case["lo"], np.float64), np.asarray(case["cell"], np.float64)
    for k in range(K):
        members = np.nonzero(vc == k)[0]
        assert members.min() == np.nonzero(vc == k)[0][0] and (k == 0 or members.min() > np.nonzero(vc == k - 1)[0].min())      # ids ascend in the leader
        cell_lo = lo + c[members[0]] * cell
        assert (out_v[k] >= (cell_lo - 1e-6)).all() and (out_v[k] <= cell_lo + cell * (1 + 1e-6)).all(), (name, k)
        assert (out_c[k] >= col[members].min(axis=0) - 2e-6).all() and (out_c[k] <= col[members].max(axis=0) + 2e-6).all()
        assert abs(np.linalg.norm(out_n[k].astype(np.float64)) - 1.0) < 1e-6 or not out_n[k].any()
    # without normals and colours: the same mesh, None in their places
    bare = S.cluster_ref(v, f, case["lo"], case["cell"], case["n"])
    assert bare[2] is None and bare[3] is None and np.array_equal(bare[0], out_v) and np.array_equal(bare[1], out_f) and np.array_equal(bare[4], vc)
    # the order of the faces: the kept face of a set is the first of the list it is handed
    back = S.cluster_ref(v, f[::-1], case["lo"], case["cell"], case["n"])
    assert np.array_equal(back[0], out_v) and np.array_equal(back[4], vc) and len(back[1]) == len(out_f)
    assert sorted(map(sorted, back[1].tolist())) == sorted(map(sorted, out_f.tolist()))


def test_nothing_merged_moves_a_vertex_by_less_than_the_stated_bound():
    case = S.hand("nothing merges")
    out_v, out_f, _, _, vc = S.cluster_ref(case["v"], case["f"], case["lo"], case["cell"], case["n"])
    assert vc.tolist() == [0, 1, 2, 3] and len(out_v) == len(case["v"])
    moved = np.abs(out_v.astype(np.float64) - case["v"].astype(np.float64))
    bound = 0.125 * 2.0 ** -20 + 2.0 ** -23 * 2.0          # the floor, and one float32 rounding of a coordinate below 2
    assert 0 < moved.max() < bound, moved.max()
    assert not np.array_equal(out_v, case["v"])            # which is why it is not a byte copy


def test_a_zero_normal_sum_gives_the_zero_vector():
    v = np.array([[.25, .5, .5], [.75, .5, .5], [1.5, .5, .5]], np.float32)
    nrm = np.array([[0, 0, 1], [0, 0, -1], [3, 0, 4]], np.float32)          # the first two cancel; the third is clamped to (1, 0, 1)
    out = S.cluster_ref(v, np.zeros((0, 3), np.int32), (0, 0, 0), (1, 1, 1), (2, 1, 1), normals=nrm)
    assert out[4].tolist() == [0, 0, 1] and out[2][0].tolist() == [0.0, 0.0, 0.0]
    assert np.allclose(out[2][1], [2 ** -0.5, 0, 2 ** -0.5], atol=2 ** -23, rtol=0)
    col = np.array([[-1, .25, 2], [1, .75, 2], [.5, .5, .5]], np.float32)   # clamped to [0, 1] before the sum
    out = S.cluster_ref(v, np.zeros((0, 3), np.int32), (0, 0, 0), (1, 1, 1), (2, 1, 1), colors=col)
    assert out[3].tolist() == [[0.5, 0.5, 1.0], [0.5, 0.5, 0.5]]


def test_grid_of_restates_simplify():
    v = np.array([[-1.0, 0.0, 0.5], [1.0, 0.25, 0.5]], np.float32)
    assert S.grid_of(v, 0.5) == ([-1.0, 0.0, 0.5], [0.5, 0.5, 0.5], [4, 1, 1])
    assert S.grid_of(v, (0.3, 0.1, 7.0)) == ([-1.0, 0.0, 0.5], [0.3, 0.1, 7.0], [7, 3, 1])
    assert S.grid_of(v, 2 / 128, lo=(-1, -1, -1), hi=(1, 1, 1))[2] == [128, 128, 128]
    assert geometry._cluster_cells([-1.0, 0.0, 0.5], [1.0, 0.25, 0.5], [0.3, 0.1, 7.0], "x") == [7, 3, 1]

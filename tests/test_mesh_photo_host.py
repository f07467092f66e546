"""Host-side checks of photo colours for meshes (csrc/crnerf_mesh_photo.h, staged beside the sources; ops.mesh_zbuffer, ops.mesh_photo_colors;
crnerf_amd.geometry Views / Mesh.depth_maps / photo_colors / Mesh.colorize_from_photos; no GPU needed): the staged header against
_lib.STAGED_PHOTO_SIGNATURES parameter by parameter, the exports and where they are bound, every refusal and no-op of the two entries -- each
call below is refused, or does nothing, on the host before any device work, so the pointers are never followed --, the ValueErrors of Views and
of the Python layer that fire before a device tensor is needed, and the NumPy restatement the GPU tests compare with
(tests/_mesh_photo_cases.py) held to values worked by hand."""
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

import _mesh_photo_cases as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cr-nerf-pytorch_amd", "csrc")
HEADER = "crnerf_mesh_photo.h"
ZBUF, COLORS = "crnerf_mesh_zbuffer_f32", "crnerf_mesh_photo_colors_u8"
ENTRIES = [ZBUF, COLORS]
PTR = 4096        # a non-NULL pointer that is never followed
BIG = 2 ** 31 - 1
SHAPE, NULL = -2, -1          # CRNERF_ERR_*
INF, NAN = float("inf"), float("nan")


def _fn(name):
    """Entry `name` of the built library on a handle of its own, bound as the staged table says."""
    assert os.path.exists(_lib.LIB_PATH), "libcrnerf_hip.so missing: run __graft_entry__.build()"
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, name), "%s is not exported" % name
    fn = getattr(lib, name)
    fn.restype, fn.argtypes = _lib.STAGED_PHOTO_SIGNATURES[HEADER][name]
    return fn


# ---------------------------------------------------------------- the header, the table, the binding
def test_staged_header_matches_the_staged_photo_table_parameter_by_parameter(monkeypatch):
    monkeypatch.setattr(_abi, "INCLUDE", CSRC)
    assert list(_lib.STAGED_PHOTO_SIGNATURES) == [HEADER] and os.path.exists(os.path.join(CSRC, HEADER))
    protos, table = _abi.prototypes(HEADER), _lib.STAGED_PHOTO_SIGNATURES[HEADER]
    assert list(protos) == list(table) == ENTRIES
    text = re.sub(r"/\*.*?\*/", "", _abi.header_text(HEADER), flags=re.S)
    assert sorted(set(re.findall(r"\b(crnerf_[a-z0-9_]+)\s*\(", text))) == sorted(table)      # nothing that looks like an entry escaped the parser
    assert "struct" not in text                                                                 # scalars by value, tables by device pointer
    for symbol, (ret, params) in protos.items():
        restype, argtypes = table[symbol]
        assert restype is _abi.RESTYPES[ret], symbol
        assert len(argtypes) == len(params), symbol
        for k, (decl, argtype) in enumerate(zip(params, argtypes)):
            assert argtype is _abi.expected_argtype(symbol, decl), "%s, parameter %d (%s): the table says %s" % (symbol, k, decl, argtype)
    assert [protos[n][0] for n in ENTRIES] == ["int", "int"] and [len(protos[n][1]) for n in ENTRIES] == [12, 15]
    names = {n: [d.split()[-1].lstrip("*") for d in protos[n][1]] for n in ENTRIES}
    assert names[ZBUF] == ["vertices", "faces", "V", "F", "cams", "dims", "offsets", "N", "total_pixels", "z_near", "depth", "stream"]
    assert names[COLORS] == ["vertices", "normals", "V", "photos", "depth", "cams", "dims", "offsets", "N", "total_pixels", "z_near", "depth_tol",
                             "out_colors", "out_views", "stream"]
    types = {n: [" ".join(d.split()[:-1]) for d in protos[n][1]] for n in ENTRIES}
    assert types[ZBUF][4:7] == ["const double*", "const int32_t*", "const int64_t*"] and types[ZBUF][9] == "double"
    assert types[COLORS][3] == "const uint8_t*" and types[COLORS][10:12] == ["double", "double"] and types[COLORS][13] == "int32_t*"


def test_header_states_the_rules():
    with open(os.path.join(CSRC, HEADER)) as f:
        text = f.read()
    first = text.split("*/")[0]
    assert "STAGED" in first and "include/" in first and "tests/test_host.py" in first and "STAGED_PHOTO_SIGNATURES" in first
    text = re.sub(r"\s*\n \*\s*", " ", text)      # a phrase may run over the end of a comment line
    for word in ("Arithmetic.", "-ffp-contract=off", "ties to even", "false on NaN", "Views.", "no half-pixel offset", "cams[N][16]", "dims[N][2]",
                 "offsets[N]", "Skipped views.", "W > 16384", "offsets[n] + W H > total_pixels", "never written and never counted",
                 "before it has passed these tests", "Projection", "z >= z_near", "NOT the renderer's along-ray", "Valid faces.", "never dereferenced",
                 "0x7F800000", "NO near-plane clipping", "2^20", "4 sub-pixel bits", "(16 i, 16 j)", "A == 0", "no culling", "E_0 + E_1 + E_2 = A",
                 "inclusive", "no fill rule", "perspective-correct", "atomic minimum", "order of the faces", "order of the atomics",
                 "splits a large bounding box", "at most 16 pixels", "faces the camera", "s = 1.0 + depth_tol", "+inf passes", "bilinear",
                 "W - 2", "65536", "16711680", "zeros when cnt = 0", "integer sums", "same bytes on every run", "function of the input alone",
                 "[0, 2^40]", "mesh_zbuffer: ", "mesh_photo_colors: "):
        assert word in text, word


def test_entries_are_exported_bound_and_outside_the_other_tables():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    bound = _lib.load()
    for name in ENTRIES:
        assert hasattr(lib, name), name
        assert name not in _lib.ALL_SIGNATURES and name not in _lib.EXPORTS, name
        assert all(name not in table for table in _lib.HEADER_SIGNATURES.values())
        assert all(name not in table for mapping in _lib.STAGED_MAPPINGS + (_lib.STAGED_SMOOTH_SIGNATURES,) for table in mapping.values())
        fn = getattr(bound, name)
        res, args = _lib.STAGED_PHOTO_SIGNATURES[HEADER][name]
        assert fn.restype is res and list(fn.argtypes) == args, name
    assert HEADER not in _lib.HEADER_SIGNATURES and all(HEADER not in mapping for mapping in _lib.STAGED_MAPPINGS)
    assert HEADER not in _lib.STAGED_SMOOTH_SIGNATURES and HEADER not in os.listdir(os.path.join(ROOT, "include"))
    # the pins of the earlier staged headers stand
    assert _lib.STAGED_MAPPINGS == (_lib.STAGED_SIGNATURES, _lib.STAGED_MESH_SIGNATURES)
    assert list(_lib.STAGED_SMOOTH_SIGNATURES) == ["crnerf_mesh_smooth.h"]


def test_load_names_a_missing_symbol_of_the_fourth_mapping(monkeypatch):
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setitem(_lib.STAGED_PHOTO_SIGNATURES, "crnerf_not_there.h", {"crnerf_mesh_photo_not_there_u8": (ctypes.c_int, [])})
    with pytest.raises(AttributeError, match="does not export crnerf_mesh_photo_not_there_u8, which csrc/crnerf_not_there.h declares"):
        _lib.load()
    assert _lib._lib is None      # nothing half-bound is kept (monkeypatch puts the loaded handle back)


def test_the_duplicate_check_at_import_covers_the_fourth_mapping():
    with open(os.path.join(ROOT, "cr-nerf-pytorch_amd", "_lib.py")) as f:
        source = f.read()
    row = '"crnerf_mesh_zbuffer_f32": (i32, [vp, vp, i64, i64, vp, vp, vp, i64, i64, f64, vp, vp]),'
    for other in ("crnerf_feature_points_f32", "crnerf_mesh_cluster_count_f32", "crnerf_mesh_smooth_f32", "crnerf_mesh_count_f32"):
        twice = source.replace(row, row + ' "%s": (i32, []),' % other)
        assert twice != source
        with pytest.raises(ImportError, match=other):
            exec(compile(twice, "_lib_twice.py", "exec"), {"__name__": "crnerf_lib_twice", "__file__": _lib.__file__})


def test_build_knows_the_unit_and_the_header():
    spec = importlib.util.spec_from_file_location("crnerf_build_for_mesh_photo", os.path.join(ROOT, "cr-nerf-pytorch_amd", "build.py"))
    build = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(build)
    assert "mesh_photo.hip" in build.SOURCES and os.path.exists(os.path.join(CSRC, "mesh_photo.hip"))
    assert HEADER in build.HEADERS      # an edit of the staged header rebuilds
    assert build.PER_FILE_FLAGS["mesh_photo.hip"] == ["-fhonor-nans"]      # the rules' comparisons are false on NaN
    assert "-ffp-contract=off" in build.FLAGS and "-ffast-math" not in build.FLAGS
    with open(os.path.join(CSRC, "mesh_photo.hip")) as f:
        unit = f.read()
    assert '#include "mesh_common.h"' in unit and "asm" not in re.sub(r"//[^\n]*", "", unit)
    for helper in ("load_face(", "mesh_sizes(", "mesh_launch(", "MESH_REQUIRE("):
        assert helper in unit, helper


# ---------------------------------------------------------------- refusals and no-ops of the entries
def _zbuf(V=4, F=2, N=3, total=64, z_near=1e-3, vertices=PTR, faces=PTR, cams=PTR, dims=PTR, offsets=PTR, depth=PTR):
    return _fn(ZBUF)(vertices, faces, V, F, cams, dims, offsets, N, total, z_near, depth, None)


def _colors(V=4, N=3, total=64, z_near=1e-3, tol=0.02, vertices=PTR, normals=PTR, photos=PTR, depth=PTR, cams=PTR, dims=PTR, offsets=PTR,
            out_colors=PTR, out_views=PTR):
    return _fn(COLORS)(vertices, normals, V, photos, depth, cams, dims, offsets, N, total, z_near, tol, out_colors, out_views, None)


def test_zbuffer_refuses_before_any_device_work():
    who = b"mesh_zbuffer: "
    for kw in (dict(V=-1), dict(F=-1), dict(N=-1), dict(V=-2 ** 63), dict(N=-2 ** 63)):
        assert _zbuf(**kw) == SHAPE and _last_error() == who + b"negative size", kw
    for kw in (dict(V=2 ** 31), dict(F=2 ** 31), dict(N=2 ** 31), dict(N=2 ** 63 - 1)):
        assert _zbuf(**kw) == SHAPE and _last_error().startswith(who + b"more than 2^31 - 1"), kw
    for total in (-1, 2 ** 40 + 1, 2 ** 63 - 1, -2 ** 63):
        assert _zbuf(total=total) == SHAPE and _last_error() == who + b"total_pixels outside [0, 2^40]", total
    for total in (64, 0):                                               # the scalars are judged even when there is no pixel
        for bad in (0.0, -0.0, -1.0, NAN, INF, -INF):
            assert _zbuf(total=total, z_near=bad) == SHAPE and _last_error() == who + b"a z_near that is not finite or <= 0", bad
    for V, F, N in ((0, 0, 0), (4, 2, 3), (BIG, BIG, BIG)):             # no pixel: nothing to do, nothing is looked at
        assert _fn(ZBUF)(None, None, V, F, None, None, None, N, 0, 1e-3, None, None) == 0
    for V, F, N in ((4, 2, 3), (0, 0, 0), (0, 2, 3), (4, 0, 3), (4, 2, 0), (BIG, BIG, BIG)):
        for total in (1, 64, 2 ** 40):
            assert _zbuf(V, F, N, total, depth=None) == NULL and _last_error() == who + b"depth is NULL"
    for V, F, N in ((4, 2, 3), (BIG, BIG, BIG), (1, 1, 1), (0, 2, 3)):
        for field in ("faces", "cams", "dims", "offsets") + (("vertices",) if V else ()):
            assert _zbuf(V, F, N, **{field: None}) == NULL and _last_error() == who + field.encode() + b" is NULL", (field, V, F, N)


def test_photo_colors_refuses_before_any_device_work():
    who = b"mesh_photo_colors: "
    for kw in (dict(V=-1), dict(N=-1), dict(V=-2 ** 63)):
        assert _colors(**kw) == SHAPE and _last_error() == who + b"negative size", kw
    for kw in (dict(V=2 ** 31), dict(N=2 ** 31), dict(V=2 ** 40)):
        assert _colors(**kw) == SHAPE and _last_error().startswith(who + b"more than 2^31 - 1"), kw
    for total in (-1, 2 ** 40 + 1):
        assert _colors(total=total) == SHAPE and _last_error() == who + b"total_pixels outside [0, 2^40]", total
    for V in (4, 0):                                                    # the scalars are judged even when there is no vertex
        for bad in (0.0, -1.0, NAN, INF, -INF):
            assert _colors(V, z_near=bad) == SHAPE and _last_error() == who + b"a z_near that is not finite or <= 0", bad
        for bad in (-1e-9, -1.0, NAN, INF, -INF):
            assert _colors(V, tol=bad) == SHAPE and _last_error() == who + b"a depth_tol that is not finite or < 0", bad
    for N, total, tol in ((0, 0, 0.0), (3, 64, 0.02), (BIG, 2 ** 40, 1e6)):      # no vertex: nothing to do, nothing is looked at
        assert _fn(COLORS)(None, None, 0, None, None, None, None, None, N, total, 1e-3, tol, None, None, None) == 0
    for V, N, total in ((4, 3, 64), (1, 1, 4), (BIG, BIG, 2 ** 40), (4, 0, 0), (4, 0, 64), (4, 3, 0)):
        need = ["vertices", "out_colors", "out_views"] + (["cams", "dims", "offsets"] if N else []) + (["photos"] if N and total else [])
        for field in need:
            assert _colors(V, N, total, **{field: None}) == NULL and _last_error() == who + field.encode() + b" is NULL", (field, V, N, total)


# ---------------------------------------------------------------- the Python layer
K1 = [[16.0, 0.0, 3.5], [0.0, 16.0, 3.5], [0.0, 0.0, 1.0]]


def test_views_refuses_bad_tables_before_the_device_is_needed():
    pose = P.IDENTITY.tolist()
    good = dict(Ks=[K1, K1], c2ws=[pose, pose], sizes=[(8, 8), (4, 6)])
    for bad in (dict(Ks=[K1]), dict(c2ws=[pose]), dict(sizes=[(8, 8)]), dict(Ks=[K1[:2], K1[:2]]), dict(c2ws=[P.IDENTITY[:, :3].tolist()] * 2),
                dict(sizes=[(8, 8), (4, 6, 1)]), dict(sizes=[(8, 8), (4.5, 6)]), dict(Ks="abc"), dict(sizes=[8, 8])):
        with pytest.raises(ValueError, match="Views expects"):
            geometry.Views(**dict(good, **bad))
    for bad in (NAN, INF, -INF):
        k, p = [row[:] for row in K1], [row[:] for row in pose]
        k[0][0], p[1][3] = bad, bad
        for kw in (dict(Ks=[K1, k]), dict(c2ws=[p, pose])):
            with pytest.raises(ValueError, match="not finite"):
                geometry.Views(**dict(good, **kw))
    for bad in ((1, 8), (8, 1), (0, 0), (16385, 8), (8, 16385), (-4, 8)):
        with pytest.raises(ValueError, match=r"W and H must lie in \[2, 16384\]"):
            geometry.Views(**dict(good, sizes=[(8, 8), bad]))
    # a good table, float64 kept, on the host (device="cpu": the tables alone need no GPU)
    K = np.array([K1, K1]) + np.array([[[1e-9, 0, 0], [0, 0, 0], [0, 0, 0]]] * 2)
    views = geometry.Views(K, np.stack([P.IDENTITY, P.look_at((1, 2, 3), (0, 0, 0))]), [(8, 8), (16384, 2)], device="cpu")
    assert (views.n, views.sizes, views.offsets, views.total_pixels) == (2, [(8, 8), (16384, 2)], [0, 64], 64 + 32768)
    assert views.cams.dtype == torch.float64 and views.dims.dtype == torch.int32 and views.offset_table.dtype == torch.int64
    want = np.stack([P.cam_row(16.0 + 1e-9, 16.0, 3.5, 3.5, c) for c in (P.IDENTITY, P.look_at((1, 2, 3), (0, 0, 0)))])
    assert views.cams.numpy().tobytes() == want.tobytes() and views.dims.tolist() == [[8, 8], [16384, 2]] and views.offset_table.tolist() == [0, 64]
    empty = geometry.Views([], [], [], device="cpu")
    assert (empty.n, empty.total_pixels) == (0, 0) and empty.cams.shape == (0, 16) and empty.dims.shape == (0, 2) and empty.split(torch.zeros(0)) == []


def test_views_pack_and_split_on_the_host():
    views = geometry.Views([K1, K1], [P.IDENTITY, P.IDENTITY], [(8, 6), (3, 2)], device="cpu")
    rng = np.random.default_rng(0)
    photos = [rng.integers(0, 256, (6, 8, 3), dtype=np.uint8), torch.from_numpy(rng.integers(0, 256, (2, 3, 3), dtype=np.uint8))]
    flat = views.pack(photos)
    assert flat.dtype == torch.uint8 and flat.shape == (54, 3)
    back = views.split(flat)
    assert [tuple(b.shape) for b in back] == [(6, 8, 3), (2, 3, 3)] and all(np.array_equal(b.numpy(), np.asarray(p)) for b, p in zip(back, photos))
    assert [tuple(d.shape) for d in views.split(torch.zeros(54))] == [(6, 8), (2, 3)]
    assert back[1].data_ptr() == flat.data_ptr() + 48 * 3          # views of the buffer, not copies
    for bad in ([photos[0]], [photos[0], photos[0]], [photos[0].astype(np.float32), photos[1]], [photos[0].transpose(1, 0, 2), photos[1]],
                [photos[0][:, :, 0], photos[1]]):
        with pytest.raises(ValueError, match="Views.pack"):
            views.pack(bad)
    for bad in (torch.zeros(53), torch.zeros(54, 3, 1), [1, 2]):
        with pytest.raises(ValueError, match="Views.split"):
            views.split(bad)


V4 = torch.tensor([[0.0, 0.0, -1.0], [0.25, 0.0, -1.0], [0.0, -0.25, -1.0], [0.25, -0.25, -1.0]])      # on the CPU
F2 = torch.tensor([[0, 1, 2], [1, 3, 2]], dtype=torch.int32)


def test_the_python_layer_refuses_bad_arguments_before_any_device_work():
    views = geometry.Views([K1], [P.IDENTITY], [(8, 8)], device="cpu")
    mesh = geometry.Mesh(V4, F2)
    photo = [np.zeros((8, 8, 3), np.uint8)]
    for call in (lambda: mesh.depth_maps("views"), lambda: mesh.colorize_from_photos(photo, None), lambda: geometry.photo_colors(V4, photo, [views])):
        with pytest.raises(ValueError, match="views must be a geometry.Views"):
            call()
    with pytest.raises(ValueError, match="fallback must be a"):
        mesh.colorize_from_photos(photo, views, fallback=torch.zeros(3, 3))
    for bad in (0.0, -1.0, NAN, INF):
        with pytest.raises(ValueError, match="z_near must be finite and > 0"):
            mesh.depth_maps(views, z_near=bad)
        with pytest.raises(ValueError, match="z_near must be finite and > 0"):
            mesh.colorize_from_photos(photo, views, occlusion=False, z_near=bad)
    for bad in (-0.01, NAN, INF):
        with pytest.raises(ValueError, match="depth_tol must be finite and >= 0"):
            geometry.photo_colors(V4, photo, views, depth_tol=bad)
    with pytest.raises(ValueError, match="Views.pack"):
        geometry.photo_colors(V4, [np.zeros((8, 7, 3), np.uint8)], views)
    with pytest.raises(ValueError, match="depths must be the flat buffer or the list"):
        geometry.photo_colors(V4, photo, views, depths=[torch.zeros(7, 8)])
    cams, dims, offsets = views.cams, views.dims, views.offset_table
    with pytest.raises(ValueError, match=r"cams as \[n,16\]"):
        ops.mesh_zbuffer(V4, F2, cams[:, :15], dims, offsets, 64, 1e-3)
    with pytest.raises(TypeError, match="cams must be torch.float64"):
        ops.mesh_zbuffer(V4, F2, cams.float(), dims, offsets, 64, 1e-3)
    with pytest.raises(ValueError, match="dims must have 1 rows"):
        ops.mesh_zbuffer(V4, F2, cams, dims.repeat(2, 1), offsets, 64, 1e-3)
    with pytest.raises(TypeError, match="offsets must be torch.int64"):
        ops.mesh_zbuffer(V4, F2, cams, dims, offsets.int(), 64, 1e-3)
    for bad in (-1, 2 ** 40 + 1, 1.5, True):
        with pytest.raises(ValueError, match=r"total_pixels must be an int in \[0, 2\^40\]"):
            ops.mesh_zbuffer(V4, F2, cams, dims, offsets, bad, 1e-3)
    with pytest.raises(ValueError, match="photos must have 64 rows"):
        ops.mesh_photo_colors(V4, None, torch.zeros(63, 3, dtype=torch.uint8), None, cams, dims, offsets, 64, 1e-3, 0.02)
    with pytest.raises(TypeError, match="photos must be torch.uint8"):
        ops.mesh_photo_colors(V4, None, torch.zeros(64, 3), None, cams, dims, offsets, 64, 1e-3, 0.02)
    with pytest.raises(ValueError, match="normals must have 4 rows"):
        ops.mesh_photo_colors(V4, V4[:3], torch.zeros(64, 3, dtype=torch.uint8), None, cams, dims, offsets, 64, 1e-3, 0.02)
    with pytest.raises(ValueError, match="depth must have 64 rows"):
        ops.mesh_photo_colors(V4, None, torch.zeros(64, 3, dtype=torch.uint8), torch.zeros(60), cams, dims, offsets, 64, 1e-3, 0.02)
    # good calls pass the checks and get as far as the device check
    with pytest.raises(RuntimeError, match="vertices must live on the GPU"):
        mesh.depth_maps(views)
    with pytest.raises(RuntimeError, match="vertices must live on the GPU"):
        mesh.colorize_from_photos(photo, views, occlusion=False)


def test_an_empty_mesh_is_coloured_without_a_device():
    views = geometry.Views([K1], [P.IDENTITY], [(8, 8)], device="cpu")
    e3, f0 = torch.zeros(0, 3), torch.zeros(0, 3, dtype=torch.int32)
    for mesh in (geometry.Mesh(e3, f0), geometry.Mesh(e3, F2, e3), geometry.Mesh(e3, f0, e3, e3)):
        got = mesh.colorize_from_photos([np.zeros((8, 8, 3), np.uint8)], views)
        assert got.colors.shape == (0, 3) and got.colors.dtype == torch.float32
        assert got.vertices is mesh.vertices and got.faces is mesh.faces and got.normals is mesh.normals


# ---------------------------------------------------------------- the restatement itself
@pytest.mark.parametrize("name", sorted(P.HAND))
def test_the_restatement_on_hand_cases(name):
    case = P.hand(name)
    got = P.zbuffer_ref(case["v"], case["f"], *case["tables"], case["z_near"])
    assert got.dtype == np.float32 and got.shape == (case["tables"][3],)
    assert got.tobytes() == case["depth"].tobytes(), (name, got)
    # the order of the faces, and which corner a face starts with, change nothing
    perm = np.random.default_rng(len(case["f"])).permutation(len(case["f"]))
    again = P.zbuffer_ref(case["v"], np.roll(case["f"][perm], 1, axis=1), *case["tables"], case["z_near"])
    assert again.tobytes() == got.tobytes()


def test_each_dropping_rule_of_the_hand_case_is_what_keeps_its_buffer(monkeypatch):
    """The hand buffer of "two triangles and the dropped faces" stands only while every rule that drops a face is in force: with the in-front
    test, the 2^20 bound, the degenerate test or the id test taken out of the restatement, the face that rule drops is drawn and the buffer changes."""
    case = P.hand("two triangles and the dropped faces")
    run = lambda: P.zbuffer_ref(case["v"], case["f"], *case["tables"], case["z_near"])      # noqa: E731
    assert run().tobytes() == case["depth"].tobytes()
    project = P.project_ref

    def always_in_front(x, cam, z_near):
        d, u, v, z, front = project(x, cam, z_near)
        return d, u, v, z, np.ones_like(front)
    with monkeypatch.context() as m:
        m.setattr(P, "project_ref", always_in_front)
        got = run().reshape(8, 8)
        assert got.tobytes() != case["depth"].tobytes() and got[2, 2] == 0.5      # (2,2) lies on the edge (1,1)-(3,3) of the face behind: depth 0.5
    with monkeypatch.context() as m:
        m.setattr(P, "MAX_UV", 2.0 ** 40)
        assert run().tobytes() != case["depth"].tobytes()
    only = lambda rows: P.zbuffer_ref(case["v"], case["f"][rows], *case["tables"], case["z_near"])      # noqa: E731
    assert not np.isfinite(only([2, 3, 4, 5, 6])).any()      # the five dropped faces alone draw nothing
    with monkeypatch.context() as m:
        m.setattr(P, "project_ref", always_in_front)
        assert np.isfinite(only([5])).any() and not np.isfinite(only([2, 3, 4, 6])).any()
    with monkeypatch.context() as m:
        m.setattr(P, "MAX_UV", 2.0 ** 40)
        assert np.isfinite(only([6])).any() and not np.isfinite(only([2, 3, 4, 5])).any()


def test_a_fronto_parallel_square_has_its_distance_on_every_covered_pixel():
    for d in (0.5, 1.0, 3.0, 7.25, 1000.0):
        v = np.array([P.at(1.25, 0.75, 1.0), P.at(6.5, 0.75, 1.0), P.at(6.5, 5.125, 1.0), P.at(1.25, 5.125, 1.0)], np.float64) * d
        f = np.array([[0, 1, 2], [0, 3, 2]], np.int32)
        got = P.zbuffer_ref(v.astype(np.float32), f, *P.tables([(P.HAND_CAM, 8, 8)]), 2.0 ** -4).reshape(8, 8)
        j, i = np.mgrid[0:8, 0:8]
        inside = (i >= 2) & (i <= 6) & (j >= 1) & (j <= 5)
        assert (got[inside] == np.float32(d)).all() and np.isinf(got[~inside]).all(), d


def test_projection_of_a_posed_camera_matches_the_ray_convention():
    """Pixel (i, j) of a camera looks along R ((i - cx) / fx, -(j - cy) / fy, -1): a point that far along that ray projects back to (i, j)."""
    c2w = P.look_at((1.0, -2.0, 0.5), (0.2, 0.1, -0.3))
    cam = P.cam_row(50.0, 48.0, 15.5, 11.25, c2w)
    rng = np.random.default_rng(5)
    ij = rng.uniform(0, 30, (64, 2))
    depth = rng.uniform(0.5, 4.0, 64)
    dirs = np.stack(((ij[:, 0] - 15.5) / 50.0, -(ij[:, 1] - 11.25) / 48.0, -np.ones(64)), axis=1)
    x = (c2w[:, 3][None, :] + depth[:, None] * dirs @ c2w[:, :3].T).astype(np.float32)
    _, u, v, z, front = P.project_ref(x, cam, 1e-3)
    assert front.all() and np.abs(u - ij[:, 0]).max() < 1e-3 and np.abs(v - ij[:, 1]).max() < 1e-3 and np.abs(z - depth).max() < 1e-5
    _, _, _, _, front = P.project_ref(np.array([[NAN, 0, 0], [0, INF, NAN], c2w[:, 3] + c2w[:, 2]], np.float32), cam, 1e-3)
    assert not front.any()          # a NaN, and a point behind the camera


def test_the_ramp_photo_gives_the_analytic_colour():
    W, H = 100, 80
    tables = P.tables([(P.HAND_CAM, W, H)])
    rng = np.random.default_rng(9)
    uv = np.concatenate((rng.uniform((0, 0), (W - 1, H - 1), (500, 2)), [[0, 0], [W - 1, H - 1], [W - 1, 0], [0, H - 1], [W - 1.5, H - 1.5], [17, 23]]))
    uv = np.round(uv * 256) / 256                       # on a lattice of 1/256 pixel: with depth 2 the projection is exact
    v = np.array([P.at(a, b, 2.0) for a, b in uv], np.float32)
    colors, seen = P.colors_ref(v, None, P.ramp(W, H).reshape(-1, 3), None, *tables, 1e-3, 0.02)
    assert colors.dtype == np.float32 and seen.dtype == np.int32 and (seen == 1).all()
    want = (uv[:, 0] + uv[:, 1]) / 255.0
    worst = float(np.abs(colors.astype(np.float64) - want[:, None]).max())
    print("ramp: the colours differ from (u + v) / 255 by at most %.3g (bound %.3g)" % (worst, P.RAMP_TOL))
    assert worst <= P.RAMP_TOL
    # a point outside the photo, one behind the camera and one too near see nothing: zeros
    out = np.array([P.at(-0.01, 5, 2.0), P.at(5, H - 0.99, 2.0), [0, 0, 1], P.at(5, 5, 2.0 ** -12)], np.float32)
    colors, seen = P.colors_ref(out, None, P.ramp(W, H).reshape(-1, 3), None, *tables, 1e-3, 0.02)
    assert not seen.any() and not colors.any()


def test_facing_occlusion_and_the_average_by_hand():
    """Two views of one point, photos of constant grey 50 and 101: the mean is 75.5 / 255; a normal that faces away from a view drops it, a zero
    normal drops none, and a z-buffer in front of the point drops the view unless the tolerance reaches it."""
    front_cam = P.cam_row(16.0, 16.0, 3.5, 3.5, P.IDENTITY)                                       # at the origin, looking along -z
    back_cam = P.cam_row(16.0, 16.0, 3.5, 3.5, P.look_at((0, 0, -4), (0, 0, -2), up=(0, 1, 0)))   # on the other side, looking along +z
    tables = P.tables([(front_cam, 8, 8), (back_cam, 8, 8)])
    photos = np.concatenate((np.full((64, 3), 50, np.uint8), np.full((64, 3), 101, np.uint8)))
    x = np.array([[0, 0, -2]], np.float32)
    run = lambda normals=None, depth=None, tol=0.02: P.colors_ref(x, normals, photos, depth, *tables, 1e-3, tol)      # noqa: E731
    colors, seen = run()
    assert seen.tolist() == [2] and colors.tolist() == [[np.float32(75.5 / 255)] * 3]
    colors, seen = run(np.array([[0, 0, 1]], np.float32))               # the normal looks at the first camera
    assert seen.tolist() == [1] and colors.tolist() == [[np.float32(50 / 255)] * 3]
    colors, seen = run(np.array([[0, 0, -1]], np.float32))
    assert seen.tolist() == [1] and colors.tolist() == [[np.float32(101 / 255)] * 3]
    assert run(np.zeros((1, 3), np.float32))[1].tolist() == [2]         # a zero normal is no opinion
    assert run(np.array([[1, 0, 0]], np.float32))[1].tolist() == [0]    # edge-on: g = 0 is not > 0
    depth = np.full(128, np.inf, np.float32)
    depth[:64] = 1.9                                                    # something 5 % nearer in the first view
    assert run(depth=depth)[1].tolist() == [1] and run(depth=depth, tol=0.06)[1].tolist() == [2]
    depth[:64] = 2.0
    assert run(depth=depth, tol=0.0)[1].tolist() == [2]                 # the surface itself passes at tolerance 0

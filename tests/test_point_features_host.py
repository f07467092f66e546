"""Host-side checks of the point-feature query (csrc/crnerf_point_features.h, staged beside the sources; crnerf_amd.geometry; no GPU needed): the
staged header against _lib.STAGED_SIGNATURES parameter by parameter, the exports, every refusal and no-op of the two entries -- each call below is
refused, or does nothing, on the host before any device work, so the pointers are never followed --, the refusals of the Python layer that fire
before a device tensor is needed, and the colour slot of Mesh down to the bytes of save_ply."""
import ctypes
import importlib.util
import os
import re
import struct

import pytest
import torch

import _abi
from crnerf_amd import _lib, geometry, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cr-nerf-pytorch_amd", "csrc")
HEADER = "crnerf_point_features.h"
ENTRIES = ["crnerf_feature_points_f32", "crnerf_feature_points_bf16"]
P = 4096          # a non-NULL pointer that is never followed
BIG = 2 ** 31 - 1


def _fn(name):
    """Entry `name` of the built library on a handle of its own, bound as the staged table says."""
    assert os.path.exists(_lib.LIB_PATH), "libcrnerf_hip.so missing: run __graft_entry__.build()"
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, name), "%s is not exported" % name
    fn = getattr(lib, name)
    fn.restype, fn.argtypes = _lib.STAGED_SIGNATURES[HEADER][name]
    return fn


def test_staged_header_matches_the_staged_table_parameter_by_parameter(monkeypatch):
    monkeypatch.setattr(_abi, "INCLUDE", CSRC)
    assert list(_lib.STAGED_SIGNATURES) == [HEADER] and os.path.exists(os.path.join(CSRC, HEADER))
    protos, table = _abi.prototypes(HEADER), _lib.STAGED_SIGNATURES[HEADER]
    assert list(protos) == list(table) == ENTRIES
    text = re.sub(r"/\*.*?\*/", "", _abi.header_text(HEADER), flags=re.S)
    assert sorted(set(re.findall(r"\b(crnerf_[a-z0-9_]+)\s*\(", text))) == sorted(table)      # nothing that looks like an entry escaped the parser
    for symbol, (ret, params) in protos.items():
        restype, argtypes = table[symbol]
        assert restype is _abi.RESTYPES[ret] and ret == "int", symbol
        assert [d.split()[-1] for d in params] == ["packed", "xyz", "dirs", "feature", "sigma", "n", "stream"], symbol
        assert len(argtypes) == len(params) == 7, symbol
        for k, (decl, argtype) in enumerate(zip(params, argtypes)):
            assert argtype is _abi.expected_argtype(symbol, decl), "%s, parameter %d (%s): the table says %s" % (symbol, k, decl, argtype)
        assert argtypes[5] is ctypes.c_int64 and argtypes[6] is ctypes.c_void_p      # n, stream


def test_entries_are_exported_bound_and_outside_the_counted_registry():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    bound = _lib.load()
    for name in ENTRIES:
        assert hasattr(lib, name), name
        assert name not in _lib.ALL_SIGNATURES and name not in _lib.EXPORTS, name
        assert all(name not in table for table in _lib.HEADER_SIGNATURES.values())
        fn = getattr(bound, name)
        res, args = _lib.STAGED_SIGNATURES[HEADER][name]
        assert fn.restype is res and list(fn.argtypes) == args, name
    assert HEADER not in _lib.HEADER_SIGNATURES and HEADER not in os.listdir(os.path.join(ROOT, "include"))
    # the header says where it is going
    with open(os.path.join(CSRC, HEADER)) as f:
        first = f.read().split("*/")[0]
    assert "STAGED" in first and "include/" in first and "154 rows" in first and "tests/test_host.py" in first


def test_load_names_a_missing_staged_symbol(monkeypatch):
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setitem(_lib.STAGED_SIGNATURES, "crnerf_not_there.h", {"crnerf_not_there_f32": (ctypes.c_int, [])})
    with pytest.raises(AttributeError, match="does not export crnerf_not_there_f32, which csrc/crnerf_not_there.h declares"):
        _lib.load()
    assert _lib._lib is None      # nothing half-bound is kept (monkeypatch puts the loaded handle back)


def test_build_and_audit_know_the_new_units_and_the_header():
    def load(name, path):
        spec = importlib.util.spec_from_file_location(name, path)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        return mod
    build = load("crnerf_build_for_point_features", os.path.join(ROOT, "cr-nerf-pytorch_amd", "build.py"))
    audit = load("crnerf_isa_audit_for_point_features", os.path.join(ROOT, "tools", "isa_audit.py"))
    assert HEADER in build.HEADERS      # an edit of the staged header rebuilds
    for unit in ("feature_query16.hip", "feature_query_bf16p.hip"):
        assert unit in build.SOURCES and unit in audit.AUDITED_UNITS
        assert os.path.exists(os.path.join(CSRC, unit))
    assert build.PER_FILE_FLAGS["feature_query_bf16p.hip"] == build.PER_FILE_FLAGS["mlp_forward_bf16p.hip"]      # its sibling's flags
    assert "feature_query16.hip" not in build.PER_FILE_FLAGS and "mlp_forward16.hip" not in build.PER_FILE_FLAGS


@pytest.mark.parametrize("name", ENTRIES)
def test_entry_refuses_before_any_device_work(name):
    fn, last_error = _fn(name), _abi.last_error
    assert fn(None, None, None, None, None, 0, None) == 0                      # n == 0: nothing to do, nothing is looked at
    assert fn(P, P, P, P, P, 0, None) == 0
    for n in (-1, -2 ** 40):
        assert fn(P, P, P, P, P, n, None) == -2                                # CRNERF_ERR_SHAPE
        assert last_error() == b"feature_points: negative n"
        assert fn(None, None, None, None, None, n, None) == -2                 # the shape is judged before the pointers
    for n in (2 ** 31, 2 ** 40):
        assert fn(P, P, P, P, P, n, None) == -2
        assert last_error().startswith(b"feature_points: more than 2^31 - 1 points")
        assert fn(P, P, P, P, None, n, None) == -2
    for k, field in enumerate((b"packed", b"xyz", b"dirs", b"feature")):
        for n in (1, BIG):
            for sigma in (P, None):                                            # sigma may be NULL: it is not what is refused
                a = [P, P, P, P]
                a[k] = None
                assert fn(*a, sigma, n, None) == -1, field                     # CRNERF_ERR_NULL
                assert last_error() == field + b" is NULL"


# ---------------------------------------------------------------- the Python layer
class _Model:
    """Stands where a NeRF_sigma would: no refusal below gets as far as asking it for a pack."""
    def packed_weights(self, precision="f32"):
        raise AssertionError("the call should have been refused before the pack was asked for")


class _Decoder:
    def decoder_tensors(self):
        raise AssertionError("the call should have been refused before the decoder was asked for its tensors")


OK3 = torch.zeros(5, 3)      # on the CPU


def _calls(xyz, dirs, precision="f32"):
    return (lambda: ops.feature_points(None, xyz, dirs, precision=precision),
            lambda: geometry.feature_points(_Model(), xyz, dirs, precision=precision),
            lambda: geometry.point_colors(_Model(), _Decoder(), None, xyz, dirs, precision=precision),
            lambda: geometry.Mesh(xyz, None, None).colorize(_Model(), _Decoder(), None, dirs=dirs, precision=precision))


@pytest.mark.parametrize("precision", ["f16", "f32x3", "f32h2", "auto", "bf16_hc", "bf16_fc", "fp8", ["f32"]])
def test_other_precisions_raise_naming_the_two_that_exist(precision):
    for call in _calls(None, OK3, precision):
        with pytest.raises(ValueError, match="'f32' or 'bf16'"):
            call()


@pytest.mark.parametrize("precision", ["f32", "fp32", torch.float32, "bf16", torch.bfloat16])
def test_wrong_shapes_and_mismatched_rows_raise(precision):
    for bad in (torch.zeros(5, 2), torch.zeros(5), torch.zeros(5, 3, 1), torch.zeros(3, 5)):
        for call in _calls(bad, OK3, precision):
            with pytest.raises(ValueError, match=r"xyz as \[n,3\]"):
                call()
        for call in _calls(OK3, bad, precision):
            with pytest.raises(ValueError, match=r"dirs as \[n,3\]"):
                call()
    for call in _calls(OK3, torch.zeros(4, 3), precision) + _calls(torch.zeros(0, 3), OK3, precision):
        with pytest.raises(ValueError, match="a direction per point"):
            call()
    for call in _calls([[0.0, 0.0, 0.0]], OK3, precision) + _calls(OK3, [[0.0, 0.0, 0.0]] * 5, precision):
        with pytest.raises(TypeError, match="must be a tensor"):
            call()


def test_cpu_tensors_raise():
    for call in _calls(OK3, OK3) + _calls(OK3, OK3, "bf16"):
        with pytest.raises(RuntimeError, match="xyz must live on the GPU"):
            call()
    for call in _calls(OK3.double(), OK3):      # (the device is judged before the element type)
        with pytest.raises(RuntimeError, match="xyz must live on the GPU"):
            call()


def test_colorize_without_normals_or_directions_raises():
    mesh = geometry.Mesh(OK3, torch.zeros(0, 3, dtype=torch.int32))
    assert mesh.normals is None and mesh.colors is None
    with pytest.raises(ValueError, match="no normals"):
        mesh.colorize(_Model(), _Decoder(), None)
    with pytest.raises(ValueError, match="no normals"):
        mesh.colorize(_Model(), _Decoder(), None, precision="bf16")
    with pytest.raises(RuntimeError, match="xyz must live on the GPU"):      # with normals the call gets as far as the device check
        geometry.Mesh(OK3, torch.zeros(0, 3, dtype=torch.int32), OK3).colorize(_Model(), _Decoder(), None)


# ---------------------------------------------------------------- Mesh: the colour slot and save_ply
V5 = torch.tensor([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0], [1.0, 1.0, 1.0]])
N5 = torch.tensor([[0.0, 0.0, 1.0], [0.0, 1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, -1.0], [0.0, 0.0, 0.0]])
F3 = torch.tensor([[0, 1, 2], [0, 2, 3], [1, 4, 2]], dtype=torch.int32)
C5 = torch.tensor([[0.0, 1.0, 0.5], [-0.1, 1.2, 0.25], [0.999, 0.001, 0.75], [0.5, 0.5, 0.5], [1.0, 0.0, 254.5 / 255.0]])
U5 = [[0, 255, 127], [0, 255, 63], [254, 0, 191], [127, 127, 127], [255, 0, 254]]      # (c.clamp(0, 1) * 255) truncated


def _read_ply(path):
    """(property lines of the vertex element, vertex rows as tuples, faces) of a binary little-endian PLY with float / uchar vertex properties."""
    with open(path, "rb") as f:
        blob = f.read()
    head, body = blob.split(b"end_header\n", 1)
    lines = head.decode("ascii").split("\n")
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0"
    nv = int(next(ln for ln in lines if ln.startswith("element vertex")).split()[-1])
    nf = int(next(ln for ln in lines if ln.startswith("element face")).split()[-1])
    at = lines.index(next(ln for ln in lines if ln.startswith("element vertex")))
    props = []
    for ln in lines[at + 1:]:
        if not ln.startswith("property"):
            break
        props.append(ln)
    fmt = "<" + "".join({"float": "f", "uchar": "B"}[p.split()[1]] for p in props)
    size = struct.calcsize(fmt)
    rows = [struct.unpack_from(fmt, body, i * size) for i in range(nv)]
    faces = [struct.unpack_from("<Biii", body, nv * size + 13 * i) for i in range(nf)]
    assert len(body) == nv * size + 13 * nf
    return props, rows, faces


def test_mesh_takes_colours_as_its_fourth_slot():
    m = geometry.Mesh(V5, F3, N5, C5)
    assert m.vertices is V5 and m.faces is F3 and m.normals is N5 and m.colors is C5
    assert geometry.Mesh(V5, F3, N5).colors is None and geometry.Mesh(V5, F3).colors is None and geometry.Mesh(V5, F3).normals is None
    assert geometry.Mesh(V5, F3, colors=C5).colors is C5
    assert geometry.Mesh.__slots__ == ("vertices", "faces", "normals", "colors")


@pytest.mark.parametrize("with_normals", [True, False])
def test_save_ply_writes_red_green_blue_behind_the_normals(tmp_path, with_normals):
    path = str(tmp_path / "c.ply")
    normals = N5 if with_normals else None
    geometry.Mesh(V5, F3, normals, C5).save_ply(path)
    props, rows, faces = _read_ply(path)
    floats = ["x", "y", "z"] + (["nx", "ny", "nz"] if with_normals else [])
    assert props == ["property float %s" % p for p in floats] + ["property uchar %s" % p for p in ("red", "green", "blue")]
    want = torch.cat((V5, N5), dim=1) if with_normals else V5
    for i, row in enumerate(rows):
        assert list(row[:len(floats)]) == want[i].tolist()
        assert list(row[len(floats):]) == U5[i], i      # 0 -> 0, 1 -> 255, 0.5 -> 127, -0.1 -> 0, 1.2 -> 255: clamped, times 255, truncated
    assert faces == [(3, 0, 1, 2), (3, 0, 2, 3), (3, 1, 4, 2)]
    with pytest.raises(ValueError, match="colors"):
        geometry.Mesh(V5, F3, normals, C5[:4]).save_ply(path)


@pytest.mark.parametrize("with_normals", [True, False])
def test_save_ply_without_colours_writes_the_bytes_it_wrote_before(tmp_path, with_normals):
    a, b = str(tmp_path / "a.ply"), str(tmp_path / "b.ply")
    normals = N5 if with_normals else None
    geometry.Mesh(V5, F3, normals, None).save_ply(a)
    geometry.Mesh(V5, F3, normals).save_ply(b)
    with open(a, "rb") as fa, open(b, "rb") as fb:
        got, same = fa.read(), fb.read()
    assert got == same
    # ... which are the bytes of the format as it stood: the header spelled out, float rows, 13-byte faces
    floats = ["x", "y", "z"] + (["nx", "ny", "nz"] if with_normals else [])
    header = ("ply\nformat binary_little_endian 1.0\ncomment crnerf_amd.geometry\nelement vertex 5\n" + "".join("property float %s\n" % p for p in floats)
              + "element face 3\nproperty list uchar int vertex_indices\nend_header\n")
    rows = torch.cat((V5, N5), dim=1) if with_normals else V5
    body = b"".join(struct.pack("<%df" % len(floats), *r) for r in rows.tolist()) + b"".join(struct.pack("<Biii", 3, *f) for f in F3.tolist())
    assert got == header.encode("ascii") + body

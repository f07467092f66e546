"""Host-side checks of the launches behind lean=True in the composite precisions (include/crnerf_lean_composite.h, which crnerf_lean.h includes;
no GPU needed): the header against _lib.LEAN_COMPOSITE_SIGNATURES, the exports, and every refusal -- each call below is refused, or is a no-op, on
the host before any device work, so the pointers in the argument blocks are never followed."""
import ctypes
import os
import re

import pytest

from crnerf_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COARSE = ["crnerf_render_coarse_weights_f32h2", "crnerf_render_coarse_weights_f32x3", "crnerf_render_coarse_weights_f32x3_repair",
          "crnerf_render_coarse_weights_f16"]
FINE = "crnerf_render_rays_lean_bf16_fine"
SYMBOLS = COARSE + [FINE]


def _header(name):
    with open(os.path.join(ROOT, "include", name)) as f:
        return f.read()


def test_header_declares_the_five_entries_and_matches_the_signature_table():
    text = re.sub(r"/\*.*?\*/", "", _header("crnerf_lean_composite.h"), flags=re.S)
    protos = {}
    for m in re.finditer(r"^\s*([A-Za-z_][\w\s\*]*?)\b(crnerf_\w+)\s*\(([^)]*)\)\s*;", text, flags=re.M):
        params = m.group(3).strip()
        protos[m.group(2)] = (m.group(1).strip(), 0 if params in ("", "void") else params.count(",") + 1)
    assert sorted(protos) == sorted(_lib.LEAN_COMPOSITE_SIGNATURES) == sorted(SYMBOLS)
    for name, (ret, nparams) in protos.items():
        restype, argtypes = _lib.LEAN_COMPOSITE_SIGNATURES[name]
        assert ret == "int" and restype is ctypes.c_int32, name
        assert nparams == len(argtypes) == 2, name
        assert argtypes[0] is ctypes.POINTER(_lib.RenderArgs) and argtypes[1] is ctypes.c_void_p, name
    # reachable through crnerf_lean.h, whose own two prototypes and crnerf.h stay as they are
    assert '#include "crnerf_lean_composite.h"' in _header("crnerf_lean.h")
    assert not set(SYMBOLS) & (set(_lib.SIGNATURES) | set(_lib.LEAN_SIGNATURES))
    assert "crnerf_render_coarse_weights" not in _header("crnerf.h")


def _fn(name):
    assert os.path.exists(_lib.LIB_PATH), "libcrnerf_hip.so missing: run __graft_entry__.build()"
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, name), "%s is not exported" % name
    fn = getattr(lib, name)
    fn.restype, fn.argtypes = _lib.LEAN_COMPOSITE_SIGNATURES[name]
    return fn


def _args(ni, **over):
    """Arguments that pass every check of an entry with n_importance = ni."""
    a = _lib.RenderArgs()
    a.n_rays, a.n_samples, a.n_importance = 4, 64, ni
    a.packed_coarse = a.packed_fine = a.rays = a.weights_coarse = a.feature_fine = a.depth_fine = 4096
    for k, v in over.items():
        setattr(a, k, v)
    return a


def _last_error():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    lib.crnerf_last_error.restype = ctypes.c_char_p
    return lib.crnerf_last_error()


@pytest.mark.parametrize("name", SYMBOLS)
def test_built_library_exports_the_entry_and_it_refuses_before_any_device_work(name):
    fn = _fn(name)
    ni = 128 if name == FINE else 0
    assert fn(None, None) == -1                                               # CRNERF_ERR_NULL
    assert fn(ctypes.byref(_lib.RenderArgs()), None) == 0                     # n_rays == 0: a no-op
    assert fn(ctypes.byref(_args(ni, n_samples=257)), None) == -2             # CRNERF_ERR_SHAPE
    assert fn(ctypes.byref(_args(ni, rng_flags=1)), None) == -3               # CRNERF_ERR_CONFIG: no draws in these kernels
    assert fn(ctypes.byref(_args(ni, z_coarse_out=4096)), None) == -3
    assert fn(ctypes.byref(_args(ni, weights_coarse=None)), None) == -1       # the one output of the coarse entries, the input of the fine one
    assert b"weights_coarse" in _last_error()
    if name == FINE:
        assert fn(ctypes.byref(_args(0)), None) == -2                         # there is no fine launch without a fine pass
        assert fn(ctypes.byref(_args(ni, n_samples=2)), None) == -2
        assert fn(ctypes.byref(_args(ni, packed_fine=None)), None) == -1
        assert fn(ctypes.byref(_args(ni, feature_fine=None)), None) == -1
    else:
        assert fn(ctypes.byref(_args(128)), None) == -2                       # a coarse-weights entry renders the coarse pass alone
        assert fn(ctypes.byref(_args(ni, n_samples=1)), None) == -2
        assert fn(ctypes.byref(_args(ni, packed_coarse=None)), None) == -1
    lib = ctypes.CDLL(_lib.LIB_PATH)
    lib.crnerf_abi_version.restype = ctypes.c_int
    assert lib.crnerf_abi_version() == 2


@pytest.mark.parametrize("precision", ["bf16", "f32", "bf16_hc", "nonsense"])
def test_render_coarse_weights_rejects_other_precisions_before_loading_anything(precision):
    from crnerf_amd import ops
    with pytest.raises(ValueError, match="precision"):
        ops.render_coarse_weights(None, None, 64, precision=precision)


def test_render_coarse_weights_takes_repair_x3_with_f16_only():
    from crnerf_amd import ops
    with pytest.raises(ValueError, match="repair_x3"):
        ops.render_coarse_weights(None, None, 64, precision="f32h2", repair_x3=object())

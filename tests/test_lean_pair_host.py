"""Host-side checks of the lean inference render on the pair core, crnerf_render_rays_lean_bf16 / _f16 (include/crnerf_lean.h; no GPU needed)."""
import ctypes
import os
import re

import pytest

from crnerf_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["crnerf_render_rays_lean_bf16", "crnerf_render_rays_lean_f16"]


def _prototypes():
    """{symbol: (return type, number of parameters)} of every prototype of include/crnerf_lean.h."""
    text = open(os.path.join(ROOT, "include", "crnerf_lean.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    protos = {}
    for m in re.finditer(r"^\s*([A-Za-z_][\w\s\*]*?)\b(crnerf_\w+)\s*\(([^)]*)\)\s*;", text, flags=re.M):
        params = m.group(3).strip()
        protos[m.group(2)] = (m.group(1).strip(), 0 if params in ("", "void") else params.count(",") + 1)
    return protos


def test_companion_header_matches_the_signature_table():
    protos = _prototypes()
    assert sorted(protos) == sorted(_lib.LEAN_SIGNATURES) == sorted(SYMBOLS)
    for name, (ret, nparams) in protos.items():
        restype, argtypes = _lib.LEAN_SIGNATURES[name]
        assert ret == "int" and restype is ctypes.c_int32, name
        assert nparams == len(argtypes) == 2, name
        assert argtypes[0] is ctypes.POINTER(_lib.RenderArgs) and argtypes[1] is ctypes.c_void_p, name
    assert not set(SYMBOLS) & set(_lib.SIGNATURES)            # crnerf.h and its table stay as they are
    with open(os.path.join(ROOT, "include", "crnerf.h")) as f:
        assert "crnerf_render_rays_lean_bf16" not in f.read()


def _fn(name):
    assert os.path.exists(_lib.LIB_PATH), "libcrnerf_hip.so missing: run __graft_entry__.build()"
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, name), "%s is not exported" % name
    fn = getattr(lib, name)
    fn.restype, fn.argtypes = _lib.LEAN_SIGNATURES[name]
    return fn


def _args(**over):
    """Arguments that pass every check (the pointers are never followed: each call below is refused, on the host, before any device work)."""
    a = _lib.RenderArgs()
    a.n_rays, a.n_samples, a.n_importance = 4, 64, 128
    a.packed_coarse = a.packed_fine = a.rays = a.feature_fine = a.depth_fine = 4096
    for k, v in over.items():
        setattr(a, k, v)
    return a


@pytest.mark.parametrize("name", SYMBOLS)
def test_built_library_exports_the_entry_and_it_refuses_before_any_device_work(name):
    fn = _fn(name)
    assert fn(None, None) == -1                                               # CRNERF_ERR_NULL
    assert fn(ctypes.byref(_lib.RenderArgs()), None) == 0                     # n_rays == 0: a no-op, as for the full entry
    assert fn(ctypes.byref(_args(n_importance=0)), None) == -2                # CRNERF_ERR_SHAPE: there is no lean coarse-only render
    assert fn(ctypes.byref(_args(n_samples=2)), None) == -2
    assert fn(ctypes.byref(_args(n_samples=257)), None) == -2
    assert fn(ctypes.byref(_args(rng_flags=1)), None) == -3                   # CRNERF_ERR_CONFIG: the pair core draws nothing in the kernel
    assert fn(ctypes.byref(_args(z_coarse_out=4096)), None) == -3
    assert fn(ctypes.byref(_args(packed_fine=None)), None) == -1
    lib = ctypes.CDLL(_lib.LIB_PATH)
    lib.crnerf_last_error.restype = ctypes.c_char_p
    assert b"packed_fine" in lib.crnerf_last_error()
    lib.crnerf_abi_version.restype = ctypes.c_int
    assert lib.crnerf_abi_version() == 2


@pytest.mark.parametrize("precision", ["f32x3", "f32h2", "auto"])
def test_other_precisions_keep_their_refusal(precision):
    from crnerf_amd import ops
    with pytest.raises(ValueError, match="lean=True"):       # raised before the library is loaded and before an argument is looked at
        ops.render_rays(None, None, None, 64, 128, lean=True, precision=precision)


def test_lean_and_repair_are_exclusive():
    from crnerf_amd import ops
    with pytest.raises(ValueError, match="repair_x3"):
        ops.render_rays(None, None, None, 64, 128, lean=True, precision="f16", repair_x3=(None, None))

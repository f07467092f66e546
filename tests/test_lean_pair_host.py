"""Host-side checks of the lean inference render on the pair core, crnerf_render_rays_lean_bf16 / _f16 (include/crnerf_lean.h; no GPU needed)."""
import ctypes

import pytest

import _abi
from crnerf_amd import _lib

SYMBOLS = ["crnerf_render_rays_lean_bf16", "crnerf_render_rays_lean_f16"]
TABLE = _lib.HEADER_SIGNATURES["crnerf_lean.h"]


def test_companion_header_matches_the_signature_table():
    _abi.check_header("crnerf_lean.h")
    protos = _abi.prototypes("crnerf_lean.h")
    assert list(protos) == list(TABLE) == SYMBOLS
    for name, (ret, params) in protos.items():
        restype, argtypes = TABLE[name]
        assert ret == "int" and restype is ctypes.c_int32, name
        assert len(params) == len(argtypes) == 2, name
        assert argtypes[0] is ctypes.POINTER(_lib.RenderArgs) and argtypes[1] is ctypes.c_void_p, name
    assert not set(SYMBOLS) & set(_lib.HEADER_SIGNATURES["crnerf.h"])            # crnerf.h and its table stay as they are
    assert "crnerf_render_rays_lean_bf16" not in _abi.header_text("crnerf.h")


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
    fn = _abi.bound(name)
    assert fn(None, None) == -1                                               # CRNERF_ERR_NULL
    assert fn(ctypes.byref(_lib.RenderArgs()), None) == 0                     # n_rays == 0: a no-op, as for the full entry
    assert fn(ctypes.byref(_args(n_importance=0)), None) == -2                # CRNERF_ERR_SHAPE: there is no lean coarse-only render
    assert fn(ctypes.byref(_args(n_samples=2)), None) == -2
    assert fn(ctypes.byref(_args(n_samples=257)), None) == -2
    assert fn(ctypes.byref(_args(rng_flags=1)), None) == -3                   # CRNERF_ERR_CONFIG: the pair core draws nothing in the kernel
    assert fn(ctypes.byref(_args(z_coarse_out=4096)), None) == -3
    assert fn(ctypes.byref(_args(packed_fine=None)), None) == -1
    assert b"packed_fine" in _abi.last_error()
    assert _abi.bound("crnerf_abi_version")() == 3


@pytest.mark.parametrize("precision", ["f32x3", "f32h2", "auto"])
def test_other_precisions_keep_their_refusal(precision):
    from crnerf_amd import ops
    with pytest.raises(ValueError, match="lean=True"):       # raised before the library is loaded and before an argument is looked at
        ops.render_rays(None, None, None, 64, 128, lean=True, precision=precision)


def test_lean_and_repair_are_exclusive():
    from crnerf_amd import ops
    with pytest.raises(ValueError, match="repair_x3"):
        ops.render_rays(None, None, None, 64, 128, lean=True, precision="f16", repair_x3=(None, None))

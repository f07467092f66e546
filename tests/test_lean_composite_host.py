"""Host-side checks of the launches behind lean=True in the composite precisions (include/crnerf_lean_composite.h, which crnerf_lean.h includes;
no GPU needed): the header against its table of _lib.HEADER_SIGNATURES, the exports, and every refusal -- each call below is refused, or is a
no-op, on the host before any device work, so the pointers in the argument blocks are never followed."""
import ctypes

import pytest

import _abi
from _abi import header_text as _header, last_error as _last_error
from crnerf_amd import _lib

COARSE = ["crnerf_render_coarse_weights_f32h2", "crnerf_render_coarse_weights_f32x3", "crnerf_render_coarse_weights_f32x3_repair",
          "crnerf_render_coarse_weights_f16"]
FINE = "crnerf_render_rays_lean_bf16_fine"
SYMBOLS = COARSE + [FINE]
TABLE = _lib.HEADER_SIGNATURES["crnerf_lean_composite.h"]


def test_header_declares_the_five_entries_and_matches_the_signature_table():
    _abi.check_header("crnerf_lean_composite.h")
    protos = _abi.prototypes("crnerf_lean_composite.h")
    assert list(protos) == list(TABLE) == SYMBOLS
    for name, (ret, params) in protos.items():
        restype, argtypes = TABLE[name]
        assert ret == "int" and restype is ctypes.c_int32, name
        assert len(params) == len(argtypes) == 2, name
        assert argtypes[0] is ctypes.POINTER(_lib.RenderArgs) and argtypes[1] is ctypes.c_void_p, name
    # reachable through crnerf_lean.h, whose own two prototypes and crnerf.h stay as they are
    assert '#include "crnerf_lean_composite.h"' in _header("crnerf_lean.h")
    assert not set(SYMBOLS) & (set(_lib.HEADER_SIGNATURES["crnerf.h"]) | set(_lib.HEADER_SIGNATURES["crnerf_lean.h"]))
    assert "crnerf_render_coarse_weights" not in _header("crnerf.h")


def _args(ni, **over):
    """Arguments that pass every check of an entry with n_importance = ni."""
    a = _lib.RenderArgs()
    a.n_rays, a.n_samples, a.n_importance = 4, 64, ni
    a.packed_coarse = a.packed_fine = a.rays = a.weights_coarse = a.feature_fine = a.depth_fine = 4096
    for k, v in over.items():
        setattr(a, k, v)
    return a


@pytest.mark.parametrize("name", SYMBOLS)
def test_built_library_exports_the_entry_and_it_refuses_before_any_device_work(name):
    fn = _abi.bound(name)
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
    assert _abi.bound("crnerf_abi_version")() == 3


@pytest.mark.parametrize("precision", ["bf16", "f32", "bf16_hc", "nonsense"])
def test_render_coarse_weights_rejects_other_precisions_before_loading_anything(precision):
    from crnerf_amd import ops
    with pytest.raises(ValueError, match="precision"):
        ops.render_coarse_weights(None, None, 64, precision=precision)


def test_render_coarse_weights_takes_repair_x3_with_f16_only():
    from crnerf_amd import ops
    with pytest.raises(ValueError, match="repair_x3"):
        ops.render_coarse_weights(None, None, 64, precision="f32h2", repair_x3=object())

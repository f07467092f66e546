"""Host-side checks of the lean render on the fp32-accurate split cores (include/crnerf_lean_x.h; no GPU needed): the header against
its table of _lib.HEADER_SIGNATURES, the exports, every refusal of the three entries -- each call below is refused, or is a no-op, on the host before any device
work, so the pointers in the argument blocks are never followed -- every refusal of ops.render_rays_lean_x that fires before a device tensor is
needed, and ops.render_rays(lean=True), which keeps refusing these precisions."""
import ctypes
import json
import os

import pytest
import torch

import _abi
from _abi import header_text as _header, last_error as _last_error
from crnerf_amd import _lib, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["crnerf_render_rays_lean_f32x3", "crnerf_render_rays_lean_f32h2", "crnerf_render_rays_lean_f32x3_repair"]
TABLE = _lib.HEADER_SIGNATURES["crnerf_lean_x.h"]


def test_header_declares_the_three_entries_and_matches_the_signature_table():
    _abi.check_header("crnerf_lean_x.h")
    protos = _abi.prototypes("crnerf_lean_x.h")
    assert list(protos) == list(TABLE) == SYMBOLS
    for name, (ret, params) in protos.items():
        restype, argtypes = TABLE[name]
        assert ret == "int" and restype is ctypes.c_int32, name
        assert len(params) == len(argtypes) == 2, name
        assert argtypes[0] is ctypes.POINTER(_lib.RenderArgs) and argtypes[1] is ctypes.c_void_p, name
    # in no other header's table (tests/test_host.py: the tables are pairwise disjoint and 152 rows in all), bound by the loader; crnerf.h does not
    # know the entries
    others = set().union(*(t for h, t in _lib.HEADER_SIGNATURES.items() if h != "crnerf_lean_x.h"))
    assert not set(SYMBOLS) & others and set(SYMBOLS) <= set(_lib.ALL_SIGNATURES)
    assert "crnerf_render_rays_lean_f32x3" not in _header("crnerf.h") and "crnerf_render_rays_lean_f32h2" not in _header("crnerf.h")


def _args(**over):
    """Arguments that pass every check of a lean entry."""
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
    assert fn(ctypes.byref(_lib.RenderArgs()), None) == 0                     # n_rays == 0: a no-op
    assert fn(ctypes.byref(_args(n_rays=-1)), None) == -2                     # CRNERF_ERR_SHAPE
    for over, text in ((dict(n_importance=0), b"n_importance must be in [1, 256]"), (dict(n_importance=257), b"n_importance must be in [1, 256]"),
                       (dict(n_samples=2), b"n_samples must be in [3, 256]"), (dict(n_samples=257), b"n_samples must be in [3, 256]")):
        assert fn(ctypes.byref(_args(**over)), None) == -2, over
        assert _last_error() == b"render_rays_lean: " + text, over
    for field in ("packed_coarse", "packed_fine", "rays", "feature_fine", "depth_fine"):
        assert fn(ctypes.byref(_args(**{field: None})), None) == -1, field
        assert _last_error() == field.encode() + b" is NULL"
    for over in (dict(rng_flags=1), dict(z_coarse_out=4096), dict(noise_coarse_out=4096), dict(noise_fine_out=4096)):
        assert fn(ctypes.byref(_args(**over)), None) == -3, over              # CRNERF_ERR_CONFIG: no draws in the lean kernels
        assert _last_error().startswith(b"render_rays_lean: no in-kernel random draws")
    assert _abi.bound("crnerf_abi_version")() == 3


# ---------------------------------------------------------------- ops.render_rays_lean_x
def _pack(name):
    """A CPU buffer with the byte size of a `name` pack (an AutoPack for "auto")."""
    if name == "auto":
        return ops.AutoPack(_pack("f32h2"), _pack("f32x3"))
    return torch.zeros(getattr(_lib.load(), ops._CORES[name].bytes)(), dtype=torch.uint8)


RAYS = torch.zeros(4, 8)      # on the CPU: the last refusal a call can reach without a device


@pytest.mark.parametrize("precision", ["f32", "bf16", "f16", "bf16_hc", "bf16_fc", "nonsense"])
def test_lean_x_rejects_other_precisions_before_loading_anything(precision):
    with pytest.raises(ValueError, match="precision"):
        ops.render_rays_lean_x(None, None, None, 64, 128, precision=precision)


@pytest.mark.parametrize("precision", ["f32x3", "f32h2", "auto"])
def test_lean_x_rejects_sample_counts_and_missing_packs_before_loading_anything(precision):
    for nc, ni, text in ((64, 0, "needs n_importance > 0"), (64, -1, "needs n_importance > 0"), (2, 128, r"n_samples in \[3, 256\]"),
                         (257, 128, r"n_samples in \[3, 256\]"), (64, 257, r"n_importance in \[1, 256\]")):
        with pytest.raises(ValueError, match=text):
            ops.render_rays_lean_x(None, None, None, nc, ni, precision=precision)
    with pytest.raises(ValueError, match="both models' packs"):
        ops.render_rays_lean_x(None, None, None, 64, 128, precision=precision)
    with pytest.raises(ValueError, match="both models' packs"):
        ops.render_rays_lean_x(object(), None, None, 64, 128, precision=precision)


def test_lean_x_rejects_packs_of_another_layout():
    x3, h2, auto = _pack("f32x3"), _pack("f32h2"), _pack("auto")
    with pytest.raises(ValueError, match="precision='auto' needs packs from pack_mlp_weights"):
        ops.render_rays_lean_x(h2, h2, RAYS, 64, 128, precision="auto")
    with pytest.raises(ValueError, match="precision='auto' needs packs from pack_mlp_weights"):
        ops.render_rays_lean_x(auto, x3, RAYS, 64, 128, precision="auto")
    with pytest.raises(ValueError, match="the f32h2 entry points need"):
        ops.render_rays_lean_x(x3, x3, RAYS, 64, 128, precision="f32h2")
    with pytest.raises(ValueError, match="the f32x3 entry points need"):
        ops.render_rays_lean_x(x3, h2, RAYS, 64, 128, precision="f32x3")
    with pytest.raises(ValueError, match="an f16 pack was handed to the f32x3 entry points"):
        ops.render_rays_lean_x(ops.F16Pack(torch.zeros(8, dtype=torch.uint8)), x3, RAYS, 64, 128, precision="f32x3")
    # a refused h2 pack: x3 throughout, whose packs are then what is checked
    with pytest.raises(ValueError, match="the f32x3 entry points need"):
        ops.render_rays_lean_x(ops.AutoPack(None, h2), auto, RAYS, 64, 128, precision="auto")


@pytest.mark.parametrize("precision", ["f32x3", "f32h2", "auto"])
def test_lean_x_with_good_packs_gets_as_far_as_the_rays(precision):
    pk = _pack(precision)
    with pytest.raises(RuntimeError, match="rays is on cpu"):
        ops.render_rays_lean_x(pk, pk, RAYS, 64, 128, precision=precision)
    with pytest.raises(RuntimeError, match="rays is on cpu"):
        ops.render_rays_lean_x(pk, pk, RAYS, 64, 128, precision=precision, want_z_fine=True, launcher=True)


# ---------------------------------------------------------------- ops.render_rays(lean=True) is untouched
@pytest.mark.parametrize("precision", ["auto", "f32x3", "f32h2"])
def test_render_rays_lean_still_refuses_these_precisions_as_recorded(precision):
    with open(os.path.join(ROOT, "tests", "golden", "render_refusals.json")) as f:
        kind, text = json.load(f)["render_rays / lean under %s" % precision]
    pk = _pack(precision)
    with pytest.raises(ValueError) as e:
        ops.render_rays(pk, pk, RAYS, 8, 4, lean=True, precision=precision)
    assert kind == "ValueError" and str(e.value) == text
    assert ops._CORES["f32x3"].render_lean is None and ops._CORES["f32h2"].render_lean is None

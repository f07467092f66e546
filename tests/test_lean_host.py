"""Host-side checks of the lean inference render, crnerf_render_rays_lean_f32 (no GPU needed)."""
import ctypes
import inspect
import os
import re

from crnerf_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOL = "crnerf_render_rays_lean_f32"


def test_lean_entry_is_declared_and_bound():
    with open(os.path.join(ROOT, "include", "crnerf.h")) as f:
        header = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    assert re.search(r"\bint\s+%s\s*\(\s*const\s+crnerf_render_args\s*\*" % SYMBOL, header), "%s is not declared in include/crnerf.h" % SYMBOL
    assert SYMBOL in _lib.EXPORTS, "%s is not in _lib.EXPORTS (build() checks the library against that list)" % SYMBOL


def test_built_library_exports_the_lean_entry_and_it_validates_before_any_device_work():
    assert os.path.exists(_lib.LIB_PATH), "libcrnerf_hip.so missing: run __graft_entry__.build()"
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, SYMBOL), SYMBOL
    fn = getattr(lib, SYMBOL)
    fn.restype, fn.argtypes = ctypes.c_int, [ctypes.POINTER(_lib.RenderArgs), ctypes.c_void_p]
    assert fn(None, None) == -1                                   # CRNERF_ERR_NULL
    a = _lib.RenderArgs()
    assert fn(ctypes.byref(a), None) == 0                         # n_rays == 0: a no-op, as for the full entry
    a.n_rays, a.n_samples, a.n_importance = 4, 64, 0
    assert fn(ctypes.byref(a), None) == -2                        # CRNERF_ERR_SHAPE: there is no lean coarse-only render
    a.n_importance, a.n_samples = 128, 2
    assert fn(ctypes.byref(a), None) == -2
    a.n_samples = 64
    assert fn(ctypes.byref(a), None) == -1                        # shapes fine, pointers missing


def test_python_layers_take_the_flag():
    from crnerf_amd import ops, pipeline, video
    assert inspect.signature(ops.render_rays).parameters["lean"].default is False
    assert inspect.signature(pipeline.render_frame).parameters["lean"].default is False
    assert inspect.signature(video.render_video).parameters["lean"].default is False

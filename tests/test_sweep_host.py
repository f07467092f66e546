"""Host-side checks of the appearance sweep, crnerf_crossray_style_stats_f32 / crnerf_crossray_decode_multi_f32 (include/crnerf_sweep.h; no GPU
needed): the header against its table of _lib.HEADER_SIGNATURES, the exports, every refusal of the two entry points (each call is refused, or is a no-op, on
the host: no pointer is followed) and the Python layer's ValueErrors, raised before the library is loaded."""
import ctypes
import re

import pytest
import torch

import _abi
from crnerf_amd import _lib

SYMBOLS = ["crnerf_crossray_decode_multi_f32", "crnerf_crossray_style_stats_f32"]
TABLE = _lib.HEADER_SIGNATURES["crnerf_sweep.h"]
P = 4096          # a non-NULL "pointer" that is never followed


def test_companion_header_matches_the_signature_table():
    _abi.check_header("crnerf_sweep.h")
    protos = _abi.prototypes("crnerf_sweep.h")
    assert sorted(protos) == sorted(TABLE) == SYMBOLS
    for name, (ret, params) in protos.items():
        restype, argtypes = TABLE[name]
        assert ret == "int" and restype is ctypes.c_int32, name
        assert len(params) == len(argtypes), name
    assert len(TABLE["crnerf_crossray_style_stats_f32"][1]) == 8
    assert TABLE["crnerf_crossray_decode_multi_f32"][1] == [ctypes.POINTER(_lib.SweepDecodeArgs), ctypes.c_void_p]
    # disjoint from crnerf.h and its table, which stay as they are
    assert not set(SYMBOLS) & set(_lib.HEADER_SIGNATURES["crnerf.h"]) and len(_lib.HEADER_SIGNATURES["crnerf.h"]) == 124
    assert not any(s in _abi.header_text("crnerf.h") for s in SYMBOLS)


def test_header_constants_and_struct_match_the_binding():
    consts = dict(re.findall(r"#define (CRNERF_SWEEP_\w+) (\d+)", _abi.header_text("crnerf_sweep.h")))
    assert int(consts["CRNERF_SWEEP_MAX_STYLES"]) == _lib.SWEEP_MAX_STYLES == 16
    assert int(consts["CRNERF_SWEEP_STATS_FLOATS"]) == _lib.SWEEP_STATS_FLOATS == 64 + 1024
    assert (int(consts["CRNERF_SWEEP_OUT_F32"]), int(consts["CRNERF_SWEEP_OUT_U8"])) == (_lib.SWEEP_OUT_F32, _lib.SWEEP_OUT_U8) == (0, 1)
    fields = _abi.struct_fields("crnerf_sweep_decode_args")
    assert [f for _, f, _ in fields] == [n for n, _ in _lib.SweepDecodeArgs._fields_]
    for (c_type, _, n), (name, ct) in zip(fields, _lib.SweepDecodeArgs._fields_):
        assert n is None and ct is _abi.expected_ctype(c_type), name
    assert _lib.SWEEP_MAX_STYLES * 196 * 4 == 12544          # the LDS the folded maps take: 12.25 KiB


def test_built_library_exports_the_entries():
    for name in SYMBOLS:
        _abi.bound(name)
    assert _abi.bound("crnerf_abi_version")() == 3


def _weights(hole=None):
    arr = (ctypes.c_void_p * 22)(*([P] * 22))
    if hole is not None:
        arr[hole] = None
    return arr


def test_style_stats_refusals():
    fn = _abi.bound("crnerf_crossray_style_stats_f32")
    w = _weights()
    ok = dict(styles=P, S=2, HWs=1024, content_HW=4096, weights=w, workspace=P, stats=P)

    def call(**over):
        a = dict(ok, **over)
        return fn(a["styles"], a["S"], a["HWs"], a["content_HW"], a["weights"], a["workspace"], a["stats"], None)
    assert call(S=0) == 0 and call(S=0, styles=None, weights=None, workspace=None, stats=None) == 0        # no-op
    for field in ("styles", "weights", "workspace", "stats"):
        assert call(**{field: None}) == -1
        assert field.encode() in _abi.last_error()
    assert call(weights=_weights(hole=7)) == -1 and b"weight" in _abi.last_error()
    assert call(S=-1) == -2 and call(HWs=-1) == -2 and call(content_HW=-1) == -2
    assert call(S=17) == -2 and b"CRNERF_SWEEP_MAX_STYLES" in _abi.last_error()
    assert call(HWs=0) == -2 and call(content_HW=0) == -2


def _args(**over):
    a = _lib.SweepDecodeArgs()
    a.content, a.HW, a.stats, a.style_HW, a.S, a.out_kind = P, 100, P, 1024, 3, 0
    a.weights, a.workspace, a.out = ctypes.cast(_weights(), ctypes.POINTER(ctypes.c_void_p)), P, P
    a.style_stride, a.plane_stride = 300, 100
    for k, v in over.items():
        setattr(a, k, v)
    return a


def test_decode_multi_refusals():
    fn = _abi.bound("crnerf_crossray_decode_multi_f32")
    call = lambda **over: fn(ctypes.byref(_args(**over)), None)      # noqa: E731
    assert fn(None, None) == -1 and b"args" in _abi.last_error()
    assert call(S=0) == 0 and call(HW=0) == 0                                                   # no-ops
    assert call(S=0, content=None, stats=None, workspace=None, out=None) == 0
    for field in ("content", "stats", "weights", "workspace", "out"):
        assert call(**{field: None}) == -1
        assert field.encode() in _abi.last_error()
    hole = _weights(hole=21)
    assert call(weights=ctypes.cast(hole, ctypes.POINTER(ctypes.c_void_p))) == -1 and b"weight" in _abi.last_error()
    assert call(S=17) == -2 and b"CRNERF_SWEEP_MAX_STYLES" in _abi.last_error()
    assert call(S=-1) == -2 and call(HW=-1) == -2 and call(style_HW=-1) == -2 and call(style_HW=0) == -2
    assert call(out_kind=2) == -3 and call(out_kind=-1) == -3 and b"out_kind" in _abi.last_error()
    assert call(plane_stride=99) == -2                       # planes overlap
    assert call(style_stride=299) == -2                      # float images overlap: 2 * 100 + 100
    assert call(out_kind=1, style_stride=299) == -2          # uint8 frames overlap: 3 * 100


# ------------------------------------------------------------------------------------------------------------------ the Python layer
@pytest.fixture
def no_library(monkeypatch):
    def load():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(_lib, "load", load)


def _w(requires_grad=False):
    return [torch.zeros(1, requires_grad=requires_grad) for _ in range(22)]


def test_style_stats_value_errors_come_before_the_library(no_library):
    from crnerf_amd import ops
    g = torch.zeros(1024, 64)
    with torch.no_grad():
        with pytest.raises(ValueError, match="GPU tensor"):
            ops.crossray_style_stats([g, g], _w(), 4096)                         # CPU tensors
        with pytest.raises(ValueError, match=r"\[HW,64\]"):
            ops.crossray_style_stats([torch.zeros(1024, 63)], _w(), 4096)
        with pytest.raises(ValueError, match=r"\[HW,64\]"):
            ops.crossray_style_stats([torch.zeros(1, 64, 32, 32)], _w(), 4096)
        with pytest.raises(ValueError, match="share one size"):
            ops.crossray_style_stats([g, torch.zeros(1023, 64)], _w(), 4096)
        with pytest.raises(ValueError, match="at least one"):
            ops.crossray_style_stats([], _w(), 4096)
        with pytest.raises(ValueError, match="content_hw"):
            ops.crossray_style_stats([g], _w(), 0)
        with pytest.raises(ValueError, match="22 decoder tensors"):
            ops.crossray_style_stats([g], _w()[:21], 4096)
    with torch.enable_grad():
        with pytest.raises(ValueError, match="inference"):
            ops.crossray_style_stats([g], _w(requires_grad=True), 4096)


def test_decode_multi_value_errors_come_before_the_library(no_library):
    from crnerf_amd import ops
    small = ops.StyleStats(torch.zeros(3, 1088), 1024, True)                     # made with content_hw <= 4096
    large = ops.StyleStats(torch.zeros(3, 1088), 1024, False)
    assert (small.S, small.style_hw, small.small_path) == (3, 1024, True)
    with torch.no_grad():
        with pytest.raises(ValueError, match="GPU tensor"):
            ops.crossray_decode_multi(torch.zeros(4096, 64), small, _w())        # CPU tensors
        with pytest.raises(ValueError, match=r"\[HW,64\]"):
            ops.crossray_decode_multi(torch.zeros(4096, 32), small, _w())
        with pytest.raises(ValueError, match=r"\[HW,64\]"):
            ops.crossray_decode_multi(torch.zeros(64, 64, 1), small, _w())
        with pytest.raises(ValueError, match="crossray_style_stats"):
            ops.crossray_decode_multi(torch.zeros(4096, 64), torch.zeros(3, 1088), _w())
        with pytest.raises(ValueError, match="another order"):
            ops.crossray_decode_multi(torch.zeros(4097, 64), small, _w())        # the other side of the reduction switch
        with pytest.raises(ValueError, match="another order"):
            ops.crossray_decode_multi(torch.zeros(4096, 64), large, _w())
        with pytest.raises(ValueError, match="another order"):                   # a large style grid puts every content size on the large path
            ops.crossray_decode_multi(torch.zeros(64, 64), ops.StyleStats(torch.zeros(1, 1088), 4097, True), _w())
        with pytest.raises(ValueError, match="22 decoder tensors"):
            ops.crossray_decode_multi(torch.zeros(4096, 64), small, _w()[:3])
    with torch.enable_grad():
        with pytest.raises(ValueError, match="inference"):
            ops.crossray_decode_multi(torch.zeros(4096, 64), small, _w(requires_grad=True))

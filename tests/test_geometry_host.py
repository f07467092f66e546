"""Host-side checks of the density query (include/crnerf_geometry.h, crnerf_amd.geometry; no GPU needed): the header against
its table of _lib.HEADER_SIGNATURES, the exports, every refusal of the four entries -- each call below is refused, or is a no-op, on the host before
any device work, so the pointers are never followed -- and the refusals of the Python layer that fire before a device tensor is needed."""
import ctypes
import importlib.util
import os

import pytest
import torch

import _abi
from _abi import bound as _fn, header_text as _header, last_error as _last_error
from crnerf_amd import _lib, geometry, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POINTS = ["crnerf_sigma_points_f32", "crnerf_sigma_points_bf16"]
GRID = ["crnerf_sigma_grid_f32", "crnerf_sigma_grid_bf16"]
TABLE = _lib.HEADER_SIGNATURES["crnerf_geometry.h"]
P = 4096          # a non-NULL pointer that is never followed
BIG = 2 ** 31 - 1


def test_header_declares_the_four_entries_and_matches_the_signature_table():
    _abi.check_header("crnerf_geometry.h")
    protos = _abi.prototypes("crnerf_geometry.h")
    assert list(protos) == list(TABLE) == POINTS + GRID
    for name, (ret, params) in protos.items():
        restype, argtypes = TABLE[name]
        assert ret == "int" and restype is ctypes.c_int32, name
        assert len(params) == len(argtypes) == (5 if name in POINTS else 9), name
        assert argtypes[-1] is ctypes.c_void_p, name                        # stream
    for name in POINTS:
        assert TABLE[name][1][3] is ctypes.c_int64       # n
    for name in GRID:
        assert TABLE[name][1][4:7] == [ctypes.c_int32] * 3     # nx, ny, nz
    # in no other header's table (tests/test_host.py: pairwise disjoint, 152 rows in all); crnerf.h does not know the entries
    assert not set(TABLE) & set().union(*(t for h, t in _lib.HEADER_SIGNATURES.items() if h != "crnerf_geometry.h"))
    assert "crnerf_sigma_" not in _header("crnerf.h")


def test_build_and_audit_know_the_new_units_and_the_header():
    def load(name, path):
        spec = importlib.util.spec_from_file_location(name, path)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        return mod
    build = load("crnerf_build_for_geometry", os.path.join(ROOT, "cr-nerf-pytorch_amd", "build.py"))
    audit = load("crnerf_isa_audit_for_geometry", os.path.join(ROOT, "tools", "isa_audit.py"))
    assert all("../../include/" + header in build.HEADERS for header in _lib.HEADER_SIGNATURES)
    for unit in ("sigma_query16.hip", "sigma_query_bf16p.hip"):
        assert unit in build.SOURCES and unit in audit.AUDITED_UNITS
    assert build.PER_FILE_FLAGS["sigma_query_bf16p.hip"] == build.PER_FILE_FLAGS["mlp_forward_bf16p.hip"]      # its sibling's flags
    assert "sigma_query16.hip" not in build.PER_FILE_FLAGS and "mlp_forward16.hip" not in build.PER_FILE_FLAGS


@pytest.mark.parametrize("name", POINTS)
def test_points_entry_refuses_before_any_device_work(name):
    fn = _fn(name)
    assert fn(None, None, None, 0, None) == 0                                  # n == 0: nothing to do, nothing is looked at
    assert fn(P, P, P, 0, None) == 0
    for n in (-1, -2 ** 40):
        assert fn(P, P, P, n, None) == -2                                      # CRNERF_ERR_SHAPE
        assert _last_error() == b"sigma_points: negative n"
    for n in (2 ** 31, 2 ** 40):
        assert fn(P, P, P, n, None) == -2
        assert _last_error().startswith(b"sigma_points: more than 2^31 - 1 points")
    for k, field in enumerate((b"packed", b"xyz", b"sigma")):
        for n in (1, BIG):
            a = [P, P, P]
            a[k] = None
            assert fn(*a, n, None) == -1, field                                # CRNERF_ERR_NULL
            assert _last_error() == field + b" is NULL"


@pytest.mark.parametrize("name", GRID)
def test_grid_entry_refuses_before_any_device_work(name):
    fn = _fn(name)
    for dims in ((0, 4, 4), (4, 0, 4), (4, 4, 0), (0, 0, 0), (0, BIG, BIG)):
        assert fn(None, None, None, None, *dims, None, None) == 0, dims         # an empty axis: nothing to do
        assert fn(P, P, P, P, *dims, P, None) == 0, dims
    for dims in ((-1, 4, 4), (4, -1, 4), (4, 4, -1), (-1, 0, 4), (-2 ** 31, 1, 1)):
        assert fn(P, P, P, P, *dims, P, None) == -2, dims                      # CRNERF_ERR_SHAPE
        assert _last_error() == b"sigma_grid: negative axis length"
    for dims in ((2 ** 16, 2 ** 15, 1), (1, 2 ** 16, 2 ** 15), (1291, 1291, 1291), (BIG, 2, 1), (BIG, BIG, BIG), (46341, 46341, 1)):
        assert fn(P, P, P, P, *dims, P, None) == -2, dims                      # nx * ny * nz > 2^31 - 1
        assert _last_error().startswith(b"sigma_grid: more than 2^31 - 1 points")
    for k, field in enumerate((b"packed", b"xs", b"ys", b"zs", b"sigma")):
        for dims in ((4, 3, 2), (BIG, 1, 1), (1, 1, BIG), (46340, 46340, 1)):   # ... and <= 2^31 - 1 gets as far as the pointers
            a = [P, P, P, P, P]
            a[k] = None
            assert fn(*a[:4], *dims, a[4], None) == -1, (field, dims)          # CRNERF_ERR_NULL
            assert _last_error() == field + b" is NULL"


# ---------------------------------------------------------------- the Python layer
class _Model:
    """Stands where a NeRF_sigma would: no refusal below gets as far as asking it for a pack."""
    def packed_weights(self, precision="f32"):
        raise AssertionError("the call should have been refused before the pack was asked for")


AX = torch.linspace(-1.0, 1.0, 4)       # on the CPU


@pytest.mark.parametrize("precision", ["f16", "f32x3", "f32h2", "auto", "bf16_hc", "bf16_fc", "fp8", ["f32"]])
def test_other_precisions_raise_naming_the_two_that_exist(precision):
    for call in (lambda: ops.sigma_points(None, None, precision=precision), lambda: ops.sigma_grid(None, None, None, None, precision=precision),
                 lambda: geometry.sigma_points(_Model(), None, precision=precision), lambda: geometry.sigma_grid(_Model(), None, None, None, precision=precision),
                 lambda: geometry.density_grid(_Model(), (0, 0, 0), (1, 1, 1), 4, precision=precision)):
        with pytest.raises(ValueError, match="'f32' or 'bf16'"):
            call()


@pytest.mark.parametrize("precision", ["f32", "fp32", torch.float32, "bf16", torch.bfloat16])
def test_wrong_shapes_raise(precision):
    for bad in (torch.zeros(5, 2), torch.zeros(5), torch.zeros(5, 3, 1), torch.zeros(3, 5)):
        with pytest.raises(ValueError, match=r"xyz as \[n,3\]"):
            ops.sigma_points(None, bad, precision=precision)
        with pytest.raises(ValueError, match=r"xyz as \[n,3\]"):
            geometry.sigma_points(_Model(), bad, precision=precision)
    for k in range(3):
        axes = [AX, AX, AX]
        axes[k] = torch.zeros(4, 1)                                            # a 2-D axis
        with pytest.raises(ValueError, match=r"the axis %s as \[n\]" % ("xs", "ys", "zs")[k]):
            ops.sigma_grid(None, *axes, precision=precision)
        with pytest.raises(ValueError, match=r"the axis %s as \[n\]" % ("xs", "ys", "zs")[k]):
            geometry.sigma_grid(_Model(), *axes, precision=precision)
    with pytest.raises(TypeError, match="must be a tensor"):
        ops.sigma_points(None, [[0.0, 0.0, 0.0]], precision=precision)


def test_cpu_tensors_raise():
    with pytest.raises(RuntimeError, match="xyz must live on the GPU"):
        ops.sigma_points(None, torch.zeros(5, 3))
    with pytest.raises(RuntimeError, match="xyz must live on the GPU"):
        geometry.sigma_points(_Model(), torch.zeros(5, 3))
    with pytest.raises(RuntimeError, match="xs must live on the GPU"):
        ops.sigma_grid(None, AX, AX, AX)
    with pytest.raises(RuntimeError, match="xs must live on the GPU"):
        geometry.sigma_grid(_Model(), AX, AX, AX, precision="bf16")


def test_the_domain_is_checked_where_the_axes_are_known():
    for k in range(3):
        for v in (64.0, -64.0, 1e3, float("nan"), float("inf")):
            axes = [AX.clone(), AX.clone(), AX.clone()]
            axes[k][2] = v
            with pytest.raises(ValueError, match=r"defined for \|v\| < 64"):
                geometry.sigma_grid(_Model(), *axes)
            lo, hi = [-1.0, -1.0, -1.0], [1.0, 1.0, 1.0]
            hi[k] = v
            with pytest.raises(ValueError, match=r"outside \|v\| < 64"):
                geometry.density_grid(_Model(), lo, hi, 8)
            with pytest.raises(ValueError, match=r"outside \|v\| < 64"):
                geometry.density_grid(_Model(), hi, lo, 8, precision="bf16")
    # just inside: the axis passes the domain check and the call gets as far as the device check
    inside = AX.clone()
    inside[3] = 63.999996
    with pytest.raises(RuntimeError, match="xs must live on the GPU"):
        geometry.sigma_grid(_Model(), inside, AX, AX)
    for bad in (0, -3, (4, 0, 4)):
        with pytest.raises(ValueError, match="resolution must be positive"):
            geometry.density_grid(_Model(), (-1, -1, -1), (1, 1, 1), bad)
    with pytest.raises(ValueError, match="3-sequences"):
        geometry.density_grid(_Model(), (-1, -1), (1, 1, 1), 4)
    with pytest.raises(ValueError, match="3-sequences"):
        geometry.density_grid(_Model(), (-1, -1, -1), (1, 1, 1), (4, 4))


def test_occupied_is_nonzero_and_three_gathers():
    """DensityGrid.occupied on a hand-made grid (CPU tensors: the object holds what it is given)."""
    xs, ys, zs = torch.tensor([0.0, 1.0, 3.0]), torch.tensor([10.0, 20.0]), torch.tensor([-5.0, -4.0, -2.0, 7.0])
    sigma = torch.zeros(4, 2, 3)
    sigma[0, 1, 2], sigma[3, 0, 1], sigma[2, 1, 0], sigma[1, 0, 0] = 2.0, 5.0, 1.0, 1.5
    g = geometry.DensityGrid(sigma, xs, ys, zs)
    assert g.occupied(1.0).tolist() == [[3.0, 20.0, -5.0], [0.0, 10.0, -4.0], [1.0, 10.0, 7.0]]       # strictly above; memory order
    assert g.occupied(5.0).shape == (0, 3) and g.occupied(-1.0).shape == (24, 3)

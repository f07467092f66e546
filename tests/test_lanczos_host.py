"""CPU-only: the Lanczos restatement (tests/_lanczos_cases.py) is Pillow's 8-bit resize byte for byte -- against the stored outputs of
Pillow itself (tests/golden/g17_lanczos.npz) and, where Pillow is installed, against Pillow live --, the package's coefficient builder
gives exactly the restatement's tables, and the device entry point refuses host tensors.  No tolerance anywhere: integers."""
import math

import numpy as np
import pytest
import torch

import _lanczos_cases as L
from crnerf_amd import ops
from crnerf_amd.datasets import images

# every (in, out) size pair a table is built for in the Lanczos tests
PAIRS = sorted({p for _, H, W, w, h, _ in L.SHAPES for p in ((W, w), (H, h)) if p[0] != p[1]} | {(700, 350), (1000, 500), (700, 87), (1000, 125)})


@pytest.fixture(scope="module")
def golden_outputs():
    return L.load_golden()


def test_blocky_references_saturate_and_stay_inside(golden_outputs):
    """Pillow's own output on the blocky inputs sits on 0 / 255 for >= 20 % of the bytes and strictly inside for >= 20 %: a kernel that
    does not clamp, or clamps wrongly, cannot pass on them."""
    for key in L.SHARES:
        ref = golden_outputs[key]
        sat = float(((ref == 0) | (ref == 255)).mean())
        print("%s: %.1f %% saturated" % (key, 100 * sat))
        assert sat >= 0.2 and 1.0 - sat >= 0.2, (key, sat)


@pytest.mark.parametrize("case", L.golden_cases(), ids=lambda c: c[0])
def test_restatement_equals_golden(case, golden_outputs):
    key, kind, seed, H, W, w, h, side = case
    got = L.resize(L.case_input(case), (w, h))
    assert got.dtype == np.uint8 and got.shape == (h, w, 3)
    assert np.array_equal(got, golden_outputs[key])


def test_restatement_equals_live_pillow():
    Image = pytest.importorskip("PIL.Image")
    todo = [(L.case_input(c), c[5], c[6]) for c in L.golden_cases()]
    photo = L.noise(7, *L.PHOTO)
    todo += [(photo, L.PHOTO[1] // d, L.PHOTO[0] // d) for d in (2, 8)]
    for a, w, h in todo:
        ref = np.asarray(Image.fromarray(a).resize((w, h), Image.LANCZOS))
        assert np.array_equal(L.resize(a, (w, h)), ref), (a.shape, w, h)


@pytest.mark.parametrize("in_size,out_size", PAIRS)
def test_coefficient_tables(in_size, out_size):
    k, bounds = images.lanczos_coeffs(in_size, out_size)
    rk, rb = L.coeffs(in_size, out_size)
    assert k.dtype == np.int32 and bounds.dtype == np.int32
    assert np.array_equal(k, rk) and np.array_equal(bounds, rb)
    # ksize and the windows as specified
    scale = in_size / out_size
    support = 3.0 * max(scale, 1.0)
    ksize = int(math.ceil(support)) * 2 + 1
    assert k.shape == (out_size, ksize) and bounds.shape == (out_size, 2)
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin, xmax = int(bounds[xx, 0]), int(bounds[xx, 1])
        assert xmin == max(int(center - support + 0.5), 0) and xmin + xmax == min(int(center + support + 0.5), in_size)
        assert 0 < xmax <= ksize and not k[xx, xmax:].any()
        assert abs(int(k[xx].sum()) - (1 << 22)) <= xmax            # normalised: the row sums to 2^22 up to one rounding per tap
    # the int32 accumulator holds the largest and the smallest sum a row can produce
    pos = np.where(k > 0, k, 0).astype(np.int64).sum(axis=1)
    neg = np.where(k < 0, k, 0).astype(np.int64).sum(axis=1)
    assert int(pos.max()) * 255 + (1 << 21) < 2 ** 31 and int(neg.min()) * 255 + (1 << 21) >= -2 ** 31


def test_coefficient_builder_rejects_empty_sizes():
    with pytest.raises(ValueError):
        images.lanczos_coeffs(0, 4)
    with pytest.raises(ValueError):
        images.lanczos_coeffs(4, 0)


def test_device_entry_point_refuses_host_tensors():
    with pytest.raises(ValueError, match="GPU"):
        ops.lanczos_resize(torch.zeros(8, 8, 3, dtype=torch.uint8), (4, 4))


def test_abi_rejects_wrong_arguments_before_any_device_work():
    """crnerf_lanczos_resize_u8 returns the library's error codes for null pointers, sizes below 1, a ksize that disagrees with the sizes and
    an unknown output mode; crnerf_lanczos_workspace_bytes is the uint8 image between the passes, 0 when at most one pass runs."""
    from crnerf_amd import _lib
    lib = _lib.load()
    assert lib.crnerf_lanczos_workspace_bytes(70, 131, 65, 35) == 70 * 65 * 3
    assert lib.crnerf_lanczos_workspace_bytes(70, 131, 131, 35) == 0 and lib.crnerf_lanczos_workspace_bytes(70, 131, 65, 70) == 0
    assert lib.crnerf_lanczos_workspace_bytes(0, 131, 65, 35) == 0
    p = 4096                                                           # a non-null, 16-byte aligned value: never dereferenced on these paths
    call = lambda *a: lib.crnerf_lanczos_resize_u8(*a, None)  # noqa: E731
    ksx, ksy = 2 * math.ceil(3 * 131 / 65) + 1, 2 * math.ceil(3 * 70 / 35) + 1
    assert call(None, 70, 131, 65, 35, p, p, ksx, p, p, ksy, 0, p, p) == -1
    assert b"NULL" in lib.crnerf_last_error()
    assert call(p, 70, 131, 65, 35, p, p, ksx, p, p, ksy, 0, None, p) == -1
    assert call(p, 70, 131, 65, 35, None, p, ksx, p, p, ksy, 0, p, p) == -1
    assert call(p, 70, 131, 65, 35, p, p, ksx, p, None, ksy, 0, p, p) == -1
    assert call(p, 70, 131, 65, 35, p, p, ksx, p, p, ksy, 0, p, None) == -1        # both passes run: the workspace is needed
    assert call(p, 70, 131, 0, 35, p, p, ksx, p, p, ksy, 0, p, p) == -2
    assert call(p, 70, 131, 65, -1, p, p, ksx, p, p, ksy, 0, p, p) == -2
    assert call(p, 70, 131, 65, 35, p, p, ksx + 2, p, p, ksy, 0, p, p) == -3
    assert call(p, 70, 131, 65, 35, p, p, ksx, p, p, ksy - 2, 0, p, p) == -3
    assert call(p, 70, 131, 65, 35, p, p, ksx, p, p, ksy, 4, p, p) == -3
    assert call(p, 70, 4000, 65, 35, p, p, 2 * math.ceil(3 * 4000 / 65) + 1, p, p, ksy, 0, p, p) == -2   # a 61x horizontal downscale: over the LDS

"""CPU-only: crnerf_amd.metrics carries the reference's names and signatures (metrics.py:4-20), refuses CPU tensors and the two
arguments no caller of the reference uses, and crnerf_image_metrics_f32 rejects NULL pointers and regions below 2x2 before it
touches a device.  The file also carries the float64 restatement of the SSIM definition (include/crnerf.h; kornia's
ssim(img1, img2, window_size=3), which is not installed anywhere this suite runs) that tests/test_gpu_metrics.py holds the kernel
to, pinned here analytically so that a wrong constant, window or border cannot hide in it."""
import ctypes
import inspect
import math
import os

import pytest
import torch
import torch.nn.functional as F

from crnerf_amd import _lib, metrics, ops

C1, C2, EPS = 0.01 ** 2, 0.03 ** 2, 1e-12
WINDOW = [0.30780134, 0.38439736, 0.30780134]


def ssim_window(dtype=torch.float64):
    x = torch.arange(-1, 2, dtype=dtype)
    g = torch.exp(-x ** 2 / (2 * 1.5 ** 2))
    return g / g.sum()


def ssim_restatement(a, b, dtype=torch.float64):
    """The SSIM map of (1,C,H,W) images a, b evaluated as the reference evaluates it (reflect pad, grouped 3x3 correlation,
    E[x^2] - mu^2), in `dtype`: float64 is the yardstick, float32 the reference's own arithmetic."""
    a, b = a.to(dtype), b.to(dtype)
    g = ssim_window(dtype)
    C = a.shape[1]
    k = (g[:, None] * g[None, :]).expand(C, 1, 3, 3).contiguous()
    f = lambda t: F.conv2d(F.pad(t, (1, 1, 1, 1), mode="reflect"), k, groups=C)  # noqa: E731
    mu1, mu2 = f(a), f(b)
    s11, s22, s12 = f(a * a) - mu1 * mu1, f(b * b) - mu2 * mu2, f(a * b) - mu1 * mu2
    return ((2 * mu1 * mu2 + C1) * (2 * s12 + C2)) / ((mu1 * mu1 + mu2 * mu2 + C1) * (s11 + s22 + C2) + EPS)


# ------------------------------------------------------------------ the mirror module
def test_metrics_mirror_reference_signatures():
    P = inspect.Parameter
    def sig(fn):
        return [(p.name, p.default) for p in inspect.signature(fn).parameters.values()]
    assert sig(metrics.mse) == [("image_pred", P.empty), ("image_gt", P.empty), ("valid_mask", None), ("reduction", "mean")]
    assert sig(metrics.psnr) == [("image_pred", P.empty), ("image_gt", P.empty), ("valid_mask", None), ("reduction", "mean")]
    assert sig(metrics.ssim) == [("image_pred", P.empty), ("image_gt", P.empty), ("reduction", "mean")]
    assert sig(metrics.image_metrics) == [("image_pred", P.empty), ("image_gt", P.empty), ("half", None), ("quantize_pred", False)]
    assert sig(ops.image_metrics) == [("pred", P.empty), ("gt", P.empty), ("roi", None), ("quantize_pred", False), ("want_map", False)]


def test_pipeline_hooks_have_the_documented_signatures():
    from crnerf_amd import pipeline
    P = inspect.Parameter
    got = [(p.name, p.default) for p in inspect.signature(pipeline.evaluate_image).parameters.values()]
    assert got == [("models", P.empty), ("embeddings", P.empty), ("enc_a", P.empty), ("sample", P.empty), ("hparams_", P.empty), ("chunk", 32768),
                   ("precision", None), ("lean", False), ("half", "right"), ("quantize_pred", True)]
    got = [(p.name, p.default) for p in inspect.signature(pipeline.TrainingSystem.validation_step).parameters.values()]
    assert got == [("self", P.empty), ("batch", P.empty), ("batch_nb", 0), ("ssim", False)]
    assert "evaluate_image" in pipeline.__all__


def test_metrics_have_no_cpu_path():
    a, b = torch.rand(1, 3, 8, 8), torch.rand(1, 3, 8, 8)
    for fn in (metrics.mse, metrics.psnr, metrics.ssim, metrics.image_metrics, ops.image_metrics):
        with pytest.raises(RuntimeError, match="GPU"):
            fn(a, b)
    with pytest.raises(RuntimeError, match="GPU"):
        metrics.psnr(torch.rand(64, 3), torch.rand(64, 3))


def test_scope_guards():
    a, b = torch.rand(1, 3, 8, 8), torch.rand(1, 3, 8, 8)
    for fn in (metrics.mse, metrics.psnr):
        with pytest.raises(NotImplementedError):
            fn(a, b, valid_mask=torch.ones(1, 3, 8, 8, dtype=torch.bool))
        with pytest.raises(NotImplementedError):
            fn(a, b, reduction="none")
    with pytest.raises(ValueError):
        metrics.image_metrics(a, b, half="left")


# ------------------------------------------------------------------ the restatement, pinned analytically
def test_window_values():
    g = ssim_window()
    assert abs(float(g.sum()) - 1.0) < 1e-15
    assert all(abs(float(g[i]) - WINDOW[i]) < 1e-7 for i in range(3))
    e = math.exp(-1.0 / 4.5)
    assert abs(float(g[0]) - e / (1 + 2 * e)) < 1e-15 and abs(float(g[1]) - 1 / (1 + 2 * e)) < 1e-15


@pytest.mark.parametrize("a,b", [(0.7, 0.7), (0.2, 0.9), (0.0, 1.0), (0.0, 0.0)])
def test_restatement_on_constant_images(a, b):
    m = ssim_restatement(torch.full((1, 3, 5, 7), a), torch.full((1, 3, 5, 7), b))
    a, b = float(torch.tensor(a, dtype=torch.float32)), float(torch.tensor(b, dtype=torch.float32))
    want = (2 * a * b + C1) * C2 / ((a * a + b * b + C1) * C2 + EPS)
    assert m.shape == (1, 3, 5, 7)
    assert float((m - want).abs().max()) <= 1e-12


def test_restatement_on_identical_images():
    a = torch.rand(1, 3, 9, 11, generator=torch.Generator().manual_seed(0)).double()
    g = ssim_window()
    k = (g[:, None] * g[None, :]).expand(3, 1, 3, 3).contiguous()
    f = lambda t: F.conv2d(F.pad(t, (1, 1, 1, 1), mode="reflect"), k, groups=3)  # noqa: E731
    mu = f(a)
    den = (2 * mu * mu + C1) * (2 * (f(a * a) - mu * mu) + C2)
    assert float((ssim_restatement(a, a) - den / (den + EPS)).abs().max()) <= 1e-12


def test_restatement_reflect_border_on_2x2():
    """2x2: every 3x3 window lies mostly in the border.  Reflect without repeating the edge maps index -1 -> 1 and 2 -> 0, so the
    window of pixel (0,0) reads rows (1,0,1) x columns (1,0,1) -- written out by hand here."""
    a = torch.tensor([[0.1, 0.9], [0.4, 0.6]], dtype=torch.float64)
    b = torch.tensor([[0.2, 0.7], [0.5, 0.3]], dtype=torch.float64)
    g = [math.exp(-1 / 4.5) / (1 + 2 * math.exp(-1 / 4.5)), 1 / (1 + 2 * math.exp(-1 / 4.5))]
    g = [g[0], g[1], g[0]]
    got = ssim_restatement(a[None, None], b[None, None])[0, 0]
    for y in range(2):
        for x in range(2):
            idx = lambda c: [1 - c, c, 1 - c]  # noqa: E731  reflected neighbours of coordinate c in a length-2 axis: (c-1, c, c+1) -> (1-c, c, 1-c)
            E = lambda fn: sum(g[j] * g[i] * fn(float(a[idx(y)[j], idx(x)[i]]), float(b[idx(y)[j], idx(x)[i]])) for j in range(3) for i in range(3))  # noqa: E731
            mu1, mu2 = E(lambda p, q: p), E(lambda p, q: q)
            s11, s22, s12 = E(lambda p, q: p * p) - mu1 * mu1, E(lambda p, q: q * q) - mu2 * mu2, E(lambda p, q: p * q) - mu1 * mu2
            want = (2 * mu1 * mu2 + C1) * (2 * s12 + C2) / ((mu1 * mu1 + mu2 * mu2 + C1) * (s11 + s22 + C2) + EPS)
            assert abs(float(got[y, x]) - want) <= 1e-12, (y, x)
    # and one value with nothing but literals: pixel (0,0), a-window mean = g0^2 (0.6*4) ... spelled out
    mu1 = g[0] * g[0] * (0.6 * 4) + g[0] * g[1] * (0.4 * 2 + 0.9 * 2) + g[1] * g[1] * 0.1
    assert abs(mu1 - (0.09474165821017468 * 2.4 + 0.11831801270312059 * 2.6 + 0.1477613163468188 * 0.1)) < 1e-12


# ------------------------------------------------------------------ the ABI without a device
def _args(w=8, h=8, width=8, height=8, x0=0, y0=0):
    a = _lib.ImageMetricsArgs()
    a.pred, a.gt = 0x1000, 0x1000                      # never dereferenced: every call below is rejected before a launch
    a.pred_stride_c, a.pred_stride_y, a.pred_stride_x = width * height, width, 1
    a.gt_stride_c, a.gt_stride_y, a.gt_stride_x = width * height, width, 1
    a.channels, a.width, a.height, a.x0, a.y0, a.w, a.h = 3, width, height, x0, y0, w, h
    return a


def test_abi_rejects_null_and_small_regions():
    lib = _lib.load()
    err = lambda: lib.crnerf_last_error().decode()  # noqa: E731
    out2, ws = ctypes.c_void_p(0x2000), ctypes.c_void_p(0x3000)
    assert lib.crnerf_image_metrics_f32(None, out2, None, ws, None) == -1 and "NULL" in err()
    assert lib.crnerf_image_metrics_f32(ctypes.byref(_args()), None, None, ws, None) == -1 and "out2" in err()
    assert lib.crnerf_image_metrics_f32(ctypes.byref(_args()), out2, None, None, None) == -1 and "workspace" in err()
    a = _args()
    a.pred = None
    assert lib.crnerf_image_metrics_f32(ctypes.byref(a), out2, None, ws, None) == -1 and "pred" in err()
    a = _args()
    a.gt = None
    assert lib.crnerf_image_metrics_f32(ctypes.byref(a), out2, None, ws, None) == -1 and "gt" in err()
    for kw in ({"w": 1}, {"h": 1}):                    # as torch's reflect pad rejects them: -1, with a message that says why
        assert lib.crnerf_image_metrics_f32(ctypes.byref(_args(**kw)), out2, None, ws, None) == -1
        assert "2x2" in err()
    for kw in ({"w": 0}, {"h": 0}, {"w": -3}):
        assert lib.crnerf_image_metrics_f32(ctypes.byref(_args(**kw)), out2, None, ws, None) != 0 and "empty" in err()
    for kw in ({"x0": 1}, {"y0": 1}, {"x0": -1}, {"w": 9}, {"x0": 4, "w": 5}):
        assert lib.crnerf_image_metrics_f32(ctypes.byref(_args(**kw)), out2, None, ws, None) != 0 and "leaves the image" in err()


def test_abi_workspace_and_tile_constants():
    lib = _lib.load()
    th, tw = ops.METRICS_TILE
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "crnerf.h")).read()
    assert "#define CRNERF_METRICS_TILE_H %d " % th in text and "#define CRNERF_METRICS_TILE_W %d\n" % tw in text
    assert lib.crnerf_image_metrics_workspace_bytes(3, tw, th) == 3 * 16              # one tile per channel, two doubles each
    assert lib.crnerf_image_metrics_workspace_bytes(3, tw + 1, th + 1) == 3 * 4 * 16
    assert lib.crnerf_image_metrics_workspace_bytes(3, 0, 5) == 0
    assert lib.crnerf_abi_version() == 3

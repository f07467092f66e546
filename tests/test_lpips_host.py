"""CPU-only: the LPIPS layer (crnerf_amd.metrics.lpips / load_lpips_weights, ops.lpips, pipeline.evaluate_lpips, crnerf_lpips_f32)
has the documented signatures, refuses CPU tensors, reads both weight-file conventions and names what is missing, and the ABI
rejects NULL pointers and regions it cannot score before it touches a device.  The float64 restatement of the definition
(tests/_lpips_cases.py) that tests/test_gpu_lpips.py holds the kernels to is pinned here analytically."""
import ctypes
import inspect

import pytest
import torch

import _lpips_cases as L
from crnerf_amd import _lib, metrics, ops, pipeline

P = inspect.Parameter


def sig(fn):
    return [(p.name, p.default) for p in inspect.signature(fn).parameters.values()]


# ------------------------------------------------------------------ the Python layer
def test_signatures():
    assert sig(ops.lpips) == [("pred", P.empty), ("gt", P.empty), ("weights", P.empty), ("roi", None), ("quantize_pred", False),
                              ("normalize", True), ("want_features", False)]
    assert sig(metrics.load_lpips_weights) == [("src", P.empty), ("lin", None), ("device", "cuda")]
    assert sig(metrics.lpips) == [("image_pred", P.empty), ("image_gt", P.empty), ("weights", P.empty), ("half", None),
                                  ("quantize_pred", False), ("normalize", True)]
    assert sig(pipeline.evaluate_lpips) == [("weights", P.empty), ("rgb", P.empty), ("sample", P.empty), ("half", "right"), ("quantize_pred", True)]
    assert {"lpips", "LPIPSWeights", "load_lpips_weights"} <= set(metrics.__all__) and "evaluate_lpips" in pipeline.__all__
    assert {"crnerf_lpips_workspace_bytes", "crnerf_lpips_f32"} <= set(_lib.EXPORTS)


def test_lpips_has_no_cpu_path():
    w = metrics.load_lpips_weights(L.lpips_state_dict(L.dead_weights()), device="cpu")
    a, b = torch.rand(1, 3, 40, 40), torch.rand(1, 3, 40, 40)
    for fn in (metrics.lpips, ops.lpips):
        with pytest.raises(RuntimeError, match="GPU"):
            fn(a, b, w)
    with pytest.raises(RuntimeError, match="GPU"):
        pipeline.evaluate_lpips(w, torch.rand(40 * 80, 3), {"rgbs": torch.rand(40 * 80, 3), "img_wh": torch.tensor([80, 40])})
    with pytest.raises(ValueError):
        metrics.lpips(a, b, w, half="left")


def test_loader_reads_both_conventions():
    ref = L.gaussian_weights(3)
    tv, lin = L.torchvision_state_dicts(ref)
    for got in (metrics.load_lpips_weights(L.lpips_state_dict(ref), device="cpu"),
                metrics.load_lpips_weights(L.lpips_state_dict(ref, lins_alias=True), device="cpu"),
                metrics.load_lpips_weights(tv, lin=lin, device="cpu")):
        assert isinstance(got, metrics.LPIPSWeights) and len(got.tensors()) == 17
        for l in range(5):
            assert torch.equal(got.conv_w[l], ref["conv_w"][l]) and torch.equal(got.conv_b[l], ref["conv_b"][l])
            assert got.lin[l].shape == (L.CHANNELS[l],) and torch.equal(got.lin[l], ref["lin"][l])
        assert all(t.dtype == torch.float32 and t.is_contiguous() and t.data_ptr() % 16 == 0 for t in got.tensors())
        assert got.shift.shape == (3,) and torch.equal(got.shift, torch.tensor(L.SHIFT)) and torch.equal(got.scale, torch.tensor(L.SCALE))
    # a dict that carries its own scaling layer wins over the defaults; one that has none gets them
    sd = L.lpips_state_dict(ref)
    sd["scaling_layer.shift"] = torch.tensor([0.1, 0.2, 0.3]).reshape(1, 3, 1, 1)
    assert torch.equal(metrics.load_lpips_weights(sd, device="cpu").shift, torch.tensor([0.1, 0.2, 0.3]))
    got = metrics.load_lpips_weights(L.lpips_state_dict(ref, scaling_layer=False), device="cpu")
    assert torch.equal(got.shift, torch.tensor((-.030, -.088, -.188))) and torch.equal(got.scale, torch.tensor((.458, .448, .450)))


def test_loader_reads_a_file(tmp_path):
    ref = L.gaussian_weights(4)
    tv, lin = L.torchvision_state_dicts(ref)
    torch.save(tv, tmp_path / "alexnet.pth")
    torch.save(lin, tmp_path / "alex.pth")
    got = metrics.load_lpips_weights(str(tmp_path / "alexnet.pth"), lin=tmp_path / "alex.pth", device="cpu")
    assert torch.equal(got.conv_w[4], ref["conv_w"][4]) and torch.equal(got.lin[2], ref["lin"][2])


def test_loader_names_what_is_wrong():
    ref = L.gaussian_weights(3)
    sd = L.lpips_state_dict(ref)
    del sd["net.slice3.6.bias"]
    with pytest.raises(KeyError, match=r"net\.slice3\.6\.bias"):
        metrics.load_lpips_weights(sd, device="cpu")
    sd = L.lpips_state_dict(ref)
    del sd["lin4.model.1.weight"]
    with pytest.raises(KeyError, match=r"lin4\.model\.1\.weight"):
        metrics.load_lpips_weights(sd, device="cpu")
    tv, lin = L.torchvision_state_dicts(ref)
    with pytest.raises(KeyError, match=r"lin0\.model\.1\.weight"):           # torchvision's file alone has no lin layers
        metrics.load_lpips_weights(tv, device="cpu")
    sd = L.lpips_state_dict(ref)
    sd["net.slice2.3.weight"] = torch.zeros(192, 64, 3, 3)
    with pytest.raises(ValueError, match=r"net\.slice2\.3\.weight"):
        metrics.load_lpips_weights(sd, device="cpu")
    lin["lin1.model.1.weight"] = torch.zeros(1, 64, 1, 1)
    with pytest.raises(ValueError, match=r"lin1\.model\.1\.weight"):
        metrics.load_lpips_weights(tv, lin=lin, device="cpu")
    sd = L.lpips_state_dict(ref)
    sd["scaling_layer.scale"] = torch.ones(4)
    with pytest.raises(ValueError, match=r"scaling_layer\.scale"):
        metrics.load_lpips_weights(sd, device="cpu")


# ------------------------------------------------------------------ the ABI without a device
def _args(w=40, h=40, width=40, height=40, x0=0, y0=0):
    a = _lib.LpipsArgs()
    a.pred, a.gt, a.shift, a.scale = 0x1000, 0x1000, 0x1000, 0x1000       # never dereferenced: every call below is rejected before a launch
    a.pred_stride_c, a.pred_stride_y, a.pred_stride_x = width * height, width, 1
    a.gt_stride_c, a.gt_stride_y, a.gt_stride_x = width * height, width, 1
    a.width, a.height, a.x0, a.y0, a.w, a.h = width, height, x0, y0, w, h
    a.normalize = 1
    for l in range(5):
        a.conv_w[l], a.conv_b[l], a.lin[l] = 0x1000, 0x1000, 0x1000
    return a


def test_abi_rejects_null_and_bad_regions():
    lib = _lib.load()
    err = lambda: lib.crnerf_last_error().decode()  # noqa: E731
    out6, ws = ctypes.c_void_p(0x2000), ctypes.c_void_p(0x3000)
    call = lambda a, o=out6, w=ws: lib.crnerf_lpips_f32(ctypes.byref(a) if a is not None else None, o, None, w, None)  # noqa: E731
    assert call(None) == -1 and "NULL" in err()
    assert call(_args(), o=None) == -1 and "out6" in err()
    assert call(_args(), w=None) == -1 and "workspace" in err()
    for field in ("pred", "gt", "shift", "scale"):
        a = _args()
        setattr(a, field, None)
        assert call(a) == -1 and field in err()
    for field in ("conv_w", "conv_b", "lin"):
        a = _args()
        getattr(a, field)[3] = None
        assert call(a) == -1 and field in err()
    for kw in ({"w": 30, "width": 30}, {"h": 30}, {"w": 30, "h": 40}):
        assert call(_args(**kw)) != 0 and "31x31" in err()
    for kw in ({"w": 0}, {"h": 0}, {"w": -3}):
        assert call(_args(**kw)) != 0 and "empty" in err()
    for kw in ({"x0": 1}, {"y0": 1}, {"x0": -1}, {"w": 41}, {"x0": 5, "w": 36}):
        assert call(_args(**kw)) != 0 and "leaves the image" in err()
    a = _args()
    a.conv_w[1] = 0x1004
    assert call(a) != 0 and "aligned" in err()
    feats = (ctypes.c_void_p * 10)(*([0x4000] * 9 + [None]))
    assert lib.crnerf_lpips_f32(ctypes.byref(_args()), out6, feats, ws, None) == -1 and "features" in err()


def test_abi_workspace_bytes():
    lib = _lib.load()
    assert lib.crnerf_lpips_workspace_bytes(0, 5) == 0
    assert lib.crnerf_lpips_workspace_bytes(30, 40) == 0 and lib.crnerf_lpips_workspace_bytes(40, 30) == 0
    small, big = lib.crnerf_lpips_workspace_bytes(31, 31), lib.crnerf_lpips_workspace_bytes(257, 340)
    # at least what the call must hold: the padded conv1 weights, conv1's patch matrix (K padded to 368) and the ten maps
    need = lambda h, w: 4 * (64 * 368 + 2 * L.map_sizes(h, w)[0][0] * L.map_sizes(h, w)[0][1] * 368  # noqa: E731
                             + 2 * sum(c * s[0] * s[1] for c, s in zip(L.CHANNELS, L.map_sizes(h, w))))
    assert small >= need(31, 31) and big >= need(340, 257) and big > small
    assert lib.crnerf_lpips_workspace_bytes(257, 340) == big and big % 256 == 0


# ------------------------------------------------------------------ the restatement, pinned analytically
@pytest.mark.parametrize("h,w,want", [(31, 31, [(7, 7), (3, 3), (1, 1)]), (63, 95, [(15, 23), (7, 11), (3, 5)]), (35, 47, [(8, 11), (3, 5), (1, 2)])])
def test_restatement_map_sizes(h, w, want):
    wts = L.gaussian_weights(1)
    f = L.features(L.scaling(torch.rand(1, 3, h, w), wts), wts)
    assert [tuple(t.shape) for t in f] == [(1, c) + s for c, s in zip(L.CHANNELS, want + [want[2], want[2]])]
    assert L.map_sizes(h, w) == want + [want[2], want[2]] == ops.lpips_map_sizes(h, w)


def test_restatement_rejects_30():
    wts = L.gaussian_weights(1)
    with pytest.raises(RuntimeError):                          # 30 -> 6 -> 2 -> no window left for the second pool
        L.features(L.scaling(torch.rand(1, 3, 30, 40), wts), wts)


def test_restatement_scaling_and_conv1_taps():
    """One tap of weight 1 at (c, ky, kx) of output channel 0 and nothing else: F1[0][oy, ox] is relu of the scaled input at
    (4 oy - 2 + ky, 4 ox - 2 + kx), 0 where that leaves the image -- stride 4, pad 2, zeros, written out by hand."""
    wts = L.dead_weights()
    wts["conv_b"][0] = torch.zeros(64)
    x = torch.rand(1, 3, 33, 37, generator=torch.Generator().manual_seed(2))
    s = (x.double() * 2 - 1 - torch.tensor(L.SHIFT).double().view(1, 3, 1, 1)) / torch.tensor(L.SCALE).double().view(1, 3, 1, 1)
    assert torch.equal(L.scaling(x, wts), s)
    assert torch.equal(L.scaling(x, wts, normalize=False), (x.double() - torch.tensor(L.SHIFT).double().view(1, 3, 1, 1))
                       / torch.tensor(L.SCALE).double().view(1, 3, 1, 1))
    for c, ky, kx in ((0, 0, 0), (1, 10, 10), (2, 2, 7), (1, 5, 1)):
        wts["conv_w"][0].zero_()
        wts["conv_w"][0][0, c, ky, kx] = 1.0
        f1 = L.features(s, wts)[0][0, 0]
        assert f1.shape == (7, 8)
        for oy in range(7):
            for ox in range(8):
                iy, ix = 4 * oy - 2 + ky, 4 * ox - 2 + kx
                want = max(float(s[0, c, iy, ix]), 0.0) if 0 <= iy < 33 and 0 <= ix < 37 else 0.0
                assert float(f1[oy, ox]) == want, (c, ky, kx, oy, ox)


def test_restatement_identities():
    wts = L.gaussian_weights(2)
    g = torch.Generator().manual_seed(0)
    a, b = torch.rand(1, 3, 40, 50, generator=g), torch.rand(1, 3, 40, 50, generator=g)
    total, d, f0, f1 = L.lpips(a, a, wts)
    assert float(total) == 0.0 and torch.equal(d, torch.zeros(5, dtype=torch.float64))
    tab, dab, _, _ = L.lpips(a, b, wts)
    tba, dba, _, _ = L.lpips(b, a, wts)
    assert float(tab) > 0 and torch.equal(dab, dba)
    # all-zero features: 0 / (0 + 1e-10) = 0, not NaN
    total, d, f0, f1 = L.lpips(a, b, L.dead_weights())
    assert all(float(t.abs().max()) == 0.0 for t in f0 + f1) and float(total) == 0.0 and not bool(torch.isnan(d).any())


def test_restatement_head_by_hand():
    """Two channels, one pixel: n0 = (3, 4) / 5, n1 = (1, 0) / 1 -> lin . (n0 - n1)^2 = 2 (0.6 - 1)^2 + 3 (0.8)^2 = 0.32 + 1.92."""
    f0, f1 = [torch.tensor([3.0, 4.0]).view(1, 2, 1, 1)], [torch.tensor([1.0, 0.0]).view(1, 2, 1, 1)]
    d = L.head(f0, f1, [torch.tensor([2.0, 3.0])])
    assert abs(float(d[0]) - 2.24) < 1e-9
    # the mean over pixels: a second pixel with identical features halves it
    f0 = [torch.tensor([[3.0, 7.0], [4.0, 7.0]]).view(1, 2, 1, 2)]
    f1 = [torch.tensor([[1.0, 7.0], [0.0, 7.0]]).view(1, 2, 1, 2)]
    assert abs(float(L.head(f0, f1, [torch.tensor([2.0, 3.0])])[0]) - 1.12) < 1e-9


def test_exact_weights_are_exactly_summable():
    """What tests/test_gpu_lpips.py's bit-for-bit test rests on: 8 entries of +-1 per row, and fp32 on the CPU already equals float64."""
    wts = L.exact_weights(5)
    for l, (cout, cin, k, _, _) in enumerate(L.LAYERS):
        rows = wts["conv_w"][l].reshape(cout, -1)
        assert bool(((rows != 0).sum(1) == 8).all()) and set(rows.unique().tolist()) == {-1.0, 0.0, 1.0}
        assert set(wts["conv_b"][l].unique().tolist()) <= {-1.0, 0.0, 1.0}
    x = torch.cat([L.exact_image(35, 47, 1), L.exact_image(35, 47, 2)], 0)
    f64 = L.features(L.scaling(x, wts, torch.float64, normalize=False), wts, torch.float64)
    f32 = L.features(L.scaling(x, wts, torch.float32, normalize=False), wts, torch.float32)
    for a, b in zip(f32, f64):
        assert torch.equal(a.double(), b) and float(b.max()) < 2 ** 17
        assert float((b * 2 - (b * 2).round()).abs().max()) == 0.0
        assert float((b != 0).double().mean()) >= 0.25

"""crnerf_lpips_f32 (csrc/lpips.hip) and the layers above it on the GPU, against the float64 restatement of the LPIPS definition
that tests/_lpips_cases.py carries and tests/test_lpips_host.py pins.

Shapes (H x W), the smallest at which the indexing can go wrong: 31x31 (conv3-5 on a 1x1 map: every tap but the centre is
padding), 35x47 (stride and pool floors drop different remainders per axis: maps 8x11, 3x5, 1x2), 63x95 (2 * 345 conv1 pixels: more
than one 32-row tile and no multiple of it), 40x95 scored on its right half (ROI 48 wide from x0 = 47), one 200x300.

1. Convolutions, bit for bit: exactly summable inputs (_lpips_cases.exact_weights / exact_image) make every partial sum in any
   order a multiple of 1/2 below 2^17, so all five maps of both images must EQUAL the float64 restatement.
2. Head: on those exact maps, with non-negative random lin, each d_l is held to the float64 head within the ABSOLUTE bound
       8 (C_l + 5) 2^-24 max(lin_l)
   (not relative: (n0 - n1)^2 cancels when the images are close).  Derivation, u = 2^-24, per pixel, all sums over the C_l channels:
   s = sum F^2 in fp32 in any order has relative error <= C u (squares and adds of positive terms); sqrt halves it and adds u, the
   + 1e-10 adds u, the division adds u: every n^ = n (1 + e), |e| <= delta = (C / 2 + 3) u.  With d = n0 - n1:
   |d^ - d| <= delta (|n0| + |n1|) + u |d|, so |d^^2 - d^2| <= 2 |d| (delta (|n0| + |n1|) + u |d|) + u d^2 to first order.  Summed with
   the weights, Cauchy-Schwarz and |n| <= 1 (so ||d|| <= 2, || |n0| + |n1| || <= 2, sum d^2 <= 4):
       sum lin 2 |d| delta (|n0| + |n1|) <= 8 delta max(lin) = (4 C + 24) u max(lin),   sum lin 3 u d^2 <= 12 u max(lin),
   and the fp32 accumulation of the C products lin * d^2 (one more rounding each) adds <= (C + 1) u * 4 max(lin).  Total
   (8 C + 40) u max(lin) per pixel; the mean over pixels is taken in double.  Measured on an MI355X (profiles/r9/lpips_parity.txt,
   the "head" lines): |d_l - float64| is 3.3e-7 ... 1.3e-4 of the bound over the 25 layer x shape cases -- the bound is a worst case
   over channels and pixels, the roundings of a real map largely cancel.
   The total is also held to the float64 head applied to the kernel's OWN returned maps under the same bound (summed over layers).
3. General weights (Gaussian, std 1.4 / sqrt(K); biases std 0.1; the package's shift / scale; uniform images): the unit is the
   reference arithmetic on the same inputs, e_ref,l = relative L2 error of the fp32 CPU restatement's F_l against float64, and the
   bar is e_hip,l <= 4 e_ref,l (a different summation order of the same K-term dot products: the four waves' K split and the MFMA's
   internal order; a wrong tap, stride, pad or pool window costs 1e-2 or more).  Both are printed per case and appended to the
   file CRNERF_LPIPS_PARITY_OUT names (profiles/r9/lpips_parity.txt: e_hip / e_ref between 0.52 and 1.29 on an MI355X).
4. Identities, bit for bit.   5. The layers above the kernel."""
import os

import pytest
import torch

import _lpips_cases as L
import _procedural_scene as scene
from crnerf_amd import metrics, ops, pipeline
from crnerf_amd.models.linearStyleTransfer import encoder_sameoutputsize

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = [(31, 31), (35, 47), (63, 95), (40, 95), (200, 300)]
U = 2.0 ** -24


def record(line):
    print(line, flush=True)
    path = os.environ.get("CRNERF_LPIPS_PARITY_OUT")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def roi_of(H, W):
    """(half, roi): 40x95 is scored on its right half, everything else whole"""
    return ("right", (W // 2, 0, W - W // 2, H)) if (H, W) == (40, 95) else (None, None)


def head_bound(lin):
    return [8 * (c + 5) * U * float(l.max()) for c, l in zip(L.CHANNELS, lin)]


_weights, _cache = {}, {}


def weights(kind):
    """(CPU dict, LPIPSWeights on the device), built once"""
    if kind not in _weights:
        w = {"exact": lambda: L.exact_weights(5, lin_seed=9), "gauss": lambda: L.gaussian_weights(11), "dead": L.dead_weights}[kind]()
        _weights[kind] = (w, metrics.load_lpips_weights(L.lpips_state_dict(w), device=DEV))
    return _weights[kind]


def case(kind, H, W):
    """Inputs and float64 (and, for 'gauss', float32) references of one case, computed once and shared (never modified)."""
    key = (kind, H, W)
    if key not in _cache:
        w, _ = weights(kind)
        half, roi = roi_of(H, W)
        x0 = roi[0] if roi else 0
        if kind == "exact":
            a, b = L.exact_image(H, W, 100 * H + W), L.exact_image(H, W, 100 * H + W + 1)
        else:
            g = torch.Generator().manual_seed(1000 * H + W)
            a, b = torch.rand(1, 3, H, W, generator=g), torch.rand(1, 3, H, W, generator=g)
        normalize = kind != "exact"
        total, d, f0, f1 = L.lpips(a[..., x0:], b[..., x0:], w, torch.float64, normalize)       # the reference crops, then scores
        c = dict(a=a, b=b, half=half, roi=roi, normalize=normalize, total=total, d=d, f=[f0, f1])
        if kind == "gauss":
            _, _, g0, g1 = L.lpips(a[..., x0:], b[..., x0:], w, torch.float32, normalize)
            c["e_ref"] = [L.rel_l2(torch.cat([p, q]), torch.cat([r, s])) for p, q, r, s in zip(g0, g1, f0, f1)]
        _cache[key] = c
    return _cache[key]


def run(kind, H, W, **kw):
    c, (_, wd) = case(kind, H, W), weights(kind)
    return ops.lpips(c["a"].to(DEV), c["b"].to(DEV), wd, roi=c["roi"], normalize=c["normalize"], **kw)


# ------------------------------------------------------------------ 1. the convolutions, bit for bit
@pytest.mark.parametrize("H,W", SHAPES)
def test_maps_equal_float64_on_exactly_summable_inputs(H, W):
    c = case("exact", H, W)
    _, _, feats = run("exact", H, W, want_features=True)
    sizes = L.map_sizes(H, c["roi"][2] if c["roi"] else W)
    for img in range(2):
        for l in range(5):
            got, want = feats[img][l].cpu(), c["f"][img][l][0]
            assert got.shape == (L.CHANNELS[l],) + sizes[l] == want.shape
            assert float((want != 0).double().mean()) >= 0.25, "dead map: the case checks nothing"
            assert torch.equal(got.double(), want), "image %d F%d: %d of %d differ, max %g" % (
                img, l + 1, int((got.double() != want).sum()), want.numel(), float((got.double() - want).abs().max()))


# ------------------------------------------------------------------ 2. the head
@pytest.mark.parametrize("H,W", SHAPES)
def test_head_within_the_operation_count_bound(H, W):
    c, (w, _) = case("exact", H, W), weights("exact")
    total, d, feats = run("exact", H, W, want_features=True)
    bound = head_bound(w["lin"])
    err = [abs(float(d[l]) - float(c["d"][l])) for l in range(5)]
    record("head  %3dx%-3d  |d_l - float64| / bound: %s   d: %s" % (H, W, " ".join("%.1e" % (e / b) for e, b in zip(err, bound)),
                                                                      " ".join("%.4f" % float(v) for v in c["d"])))
    assert total.dtype == torch.float64 and d.dtype == torch.float64 and d.shape == (5,) and total.dim() == 0
    assert float(c["total"]) > 0.05                       # two independent images: the distances are not near 0
    for l in range(5):
        assert err[l] <= bound[l], (l, err[l], bound[l])
    own = L.head([t.cpu() for t in feats[0]], [t.cpu() for t in feats[1]], w["lin"]).sum()
    assert abs(float(total) - float(own)) <= sum(bound)
    assert float(total) == float(((((d[0] + d[1]) + d[2]) + d[3]) + d[4]).cpu())     # out6[5]: the layers added in order, in double


# ------------------------------------------------------------------ 3. general weights
@pytest.mark.parametrize("H,W", SHAPES)
def test_maps_against_the_reference_arithmetic(H, W):
    c, (w, _) = case("gauss", H, W), weights("gauss")
    total, d, feats = run("gauss", H, W, want_features=True)
    e_hip = [L.rel_l2(torch.cat([feats[0][l].cpu()[None], feats[1][l].cpu()[None]]), torch.cat([c["f"][0][l], c["f"][1][l]])) for l in range(5)]
    record("maps  %3dx%-3d  e_ref: %s   e_hip: %s   lpips %.6f (float64 %.6f)" % (
        H, W, " ".join("%.2e" % e for e in c["e_ref"]), " ".join("%.2e" % e for e in e_hip), float(total), float(c["total"])))
    for l in range(5):
        assert e_hip[l] <= 4 * c["e_ref"][l], (l, e_hip[l], c["e_ref"][l])
    bound = head_bound(w["lin"])
    own = L.head([t.cpu() for t in feats[0]], [t.cpu() for t in feats[1]], w["lin"])
    for l in range(5):
        assert abs(float(d[l]) - float(own[l])) <= bound[l]


# ------------------------------------------------------------------ 4. identities, bit for bit
def same(x, y):
    return all(torch.equal(p, q) for p, q in zip(x[:2], y[:2])) and (
        x[2] is None or all(torch.equal(p, q) for i in range(2) for p, q in zip(x[2][i], y[2][i])))


@pytest.mark.parametrize("H,W", [(35, 47), (63, 95)])
def test_repeat_swap_and_self(H, W):
    c, (_, wd) = case("gauss", H, W), weights("gauss")
    a, b = c["a"].to(DEV), c["b"].to(DEV)
    first = ops.lpips(a, b, wd, want_features=True)
    assert same(first, ops.lpips(a, b, wd, want_features=True))
    swapped = ops.lpips(b, a, wd, want_features=True)
    assert torch.equal(first[0], swapped[0]) and torch.equal(first[1], swapped[1])
    assert all(torch.equal(first[2][0][l], swapped[2][1][l]) and torch.equal(first[2][1][l], swapped[2][0][l]) for l in range(5))
    total, d, _ = ops.lpips(a, a.clone(), wd)
    assert float(total) == 0.0 and torch.equal(d.cpu(), torch.zeros(5, dtype=torch.float64))
    assert float(first[0]) > 0


def test_right_half_is_the_cropped_image():
    """The left half holds values a hundred times the right half's: one read across x0 (conv1's zero padding sits AT x0) changes a map."""
    H, W = 40, 95
    c, (_, wd) = case("gauss", H, W), weights("gauss")
    x0 = W // 2
    a, b = c["a"].clone(), c["b"].clone()
    a[..., :x0] = 100 * a[..., :x0] + 50
    b[..., :x0] = -100 * b[..., :x0] - 50
    a, b = a.to(DEV), b.to(DEV)
    wide = ops.lpips(a, b, wd, roi=(x0, 0, W - x0, H), want_features=True)
    crop = ops.lpips(a[..., x0:].contiguous(), b[..., x0:].contiguous(), wd, want_features=True)
    assert same(wide, crop)
    assert same(wide, run("gauss", H, W, want_features=True))                  # and the left half's content does not matter
    assert torch.equal(metrics.lpips(a, b, wd, half="right"), crop[0].float())
    rows = ops.lpips(a, b, wd, roi=(x0 + 3, 5, 33, 31), want_features=True)     # a ROI with rows above and below it, too
    assert same(rows, ops.lpips(a[:, :, 5:36, x0 + 3:x0 + 36].contiguous(), b[:, :, 5:36, x0 + 3:x0 + 36].contiguous(), wd, want_features=True))


def test_layouts_are_read_in_place():
    H, W = 35, 47
    c, (_, wd) = case("gauss", H, W), weights("gauss")
    a, b = c["a"].to(DEV), c["b"].to(DEV)
    want = ops.lpips(a, b, wd, want_features=True)
    pm = lambda t: t[0].permute(1, 2, 0).reshape(H * W, 3).contiguous()  # noqa: E731  decode_image's [H*W,3]
    chw = lambda t: t.view(H, W, 3).permute(2, 0, 1)  # noqa: E731
    assert not chw(pm(a)).is_contiguous()
    assert same(want, ops.lpips(chw(pm(a))[None], chw(pm(b)), wd, want_features=True))
    assert same(want, ops.lpips(a[0], chw(pm(b))[None], wd, want_features=True))


def test_quantize_pred_is_the_uint8_round_trip():
    H, W = 35, 47
    c, (_, wd) = case("gauss", H, W), weights("gauss")
    raw = c["a"] * 1.2 - 0.1                                   # leaves [0,1] on both sides: the clip is part of the round trip
    png = (raw.clamp(0, 1) * 255).to(torch.uint8).float() / 255
    b = c["b"].to(DEV)
    got = ops.lpips(raw.to(DEV), b, wd, quantize_pred=True, want_features=True)
    assert same(got, ops.lpips(png.to(DEV), b, wd, want_features=True))
    assert not torch.equal(got[0], ops.lpips(raw.to(DEV), b, wd)[0])
    # the ground truth is never quantised
    assert not torch.equal(got[0], ops.lpips(b, raw.to(DEV), wd, quantize_pred=True)[0])


def test_all_zero_features_give_zero():
    c, (_, wd) = case("gauss", 35, 47), weights("dead")
    total, d, feats = ops.lpips(c["a"].to(DEV), c["b"].to(DEV), wd, want_features=True)
    assert all(float(t.abs().max()) == 0.0 for t in feats[0] + feats[1])
    assert float(total) == 0.0 and torch.equal(d.cpu(), torch.zeros(5, dtype=torch.float64))


# ------------------------------------------------------------------ 5. above the kernel
def test_metrics_lpips_is_the_total():
    H, W = 35, 47
    c, (_, wd) = case("gauss", H, W), weights("gauss")
    a, b = c["a"].to(DEV), c["b"].to(DEV)
    total, _, feats = ops.lpips(a, b, wd)
    got = metrics.lpips(a, b, wd)
    assert feats is None and got.dtype == torch.float32 and got.dim() == 0 and got.is_cuda and torch.equal(got, total.float())
    assert torch.equal(metrics.lpips(a[0], b[0], wd), got)
    assert torch.equal(metrics.lpips(a * 2 - 1, b * 2 - 1, wd, normalize=False), got)     # the same fp32 operation, done by the caller
    assert torch.equal(metrics.lpips(a, b, wd, quantize_pred=True), ops.lpips(a, b, wd, quantize_pred=True)[0].float())


def test_evaluate_lpips_on_the_procedural_scene():
    """Two views of the procedural scene side by side form one 64 x 32 test image (the left view gives the appearance, the right one is
    scored, as with a Phototourism test image): evaluate_lpips on evaluate_image's output is metrics.lpips on the same pair."""
    S = scene.SIDE
    hp = scene.hparams()
    torch.manual_seed(0)
    models, embeddings = pipeline.get_model(hp, DEV), pipeline.get_embeddings(hp)
    enc_a = encoder_sameoutputsize(out_channel=hp.nerf_out_dim).to(DEV).eval()
    for m in models.values():
        m.eval()
    views = [scene.camera_rays(0.3, 0.1), scene.camera_rays(0.8, -0.15)]
    side_by_side = lambda v: torch.cat([torch.as_tensor(v[0]).reshape(S, S, -1), torch.as_tensor(v[1]).reshape(S, S, -1)], 1).reshape(2 * S * S, -1)  # noqa: E731
    rays = side_by_side(views)
    rgbs = side_by_side([scene.ground_truth(v, n=64) for v in views]).float().clamp(0, 1)
    sample = {"rays": rays, "ts": torch.zeros(2 * S * S, dtype=torch.int64), "rgbs": rgbs,
              "whole_img": rgbs.t().reshape(3, S, 2 * S) * 2 - 1, "img_wh": torch.tensor([2 * S, S])}
    out = pipeline.evaluate_image(models, embeddings, enc_a, sample, hp, chunk=1024)
    _, wd = weights("gauss")
    got = pipeline.evaluate_lpips(wd, out["rgb"], sample)
    chw = lambda t: t.view(S, 2 * S, 3).permute(2, 0, 1)[None]  # noqa: E731
    want = metrics.lpips(chw(out["rgb"]), chw(rgbs.to(DEV)), wd, half="right", quantize_pred=True)
    assert got.dim() == 0 and got.is_cuda and got.dtype == torch.float32 and torch.equal(got, want)
    assert float(got) > 0 and float(got) == float(got)
    # the reference's protocol spelled out: PNG round trip ON THE HOST (eval.py:296-297 + ToTensor: a true division, which a division by
    # a scalar on the device is not), right half cropped to a copy, * 2 - 1 by the caller
    png = ((out["rgb"].cpu().view(S, 2 * S, 3).clamp(0, 1) * 255).to(torch.uint8).float() / 255)[:, S:].permute(2, 0, 1).contiguous().to(DEV)
    gt = rgbs.to(DEV).view(S, 2 * S, 3)[:, S:].permute(2, 0, 1).contiguous()
    assert torch.equal(got, metrics.lpips(png * 2 - 1, gt * 2 - 1, wd, normalize=False))
    whole = pipeline.evaluate_lpips(wd, out["rgb"], sample, half=None, quantize_pred=False)
    assert not torch.equal(whole, got)


def test_wrapper_rejects_what_the_kernel_cannot_read():
    _, wd = weights("gauss")
    a, b = torch.rand(1, 3, 40, 40, device=DEV), torch.rand(1, 3, 40, 40, device=DEV)
    with pytest.raises(TypeError):
        ops.lpips(a.double(), b, wd)
    with pytest.raises(TypeError):
        metrics.lpips(a, b.double(), wd)
    with pytest.raises(ValueError):
        ops.lpips(a, b[..., :39], wd)
    with pytest.raises(ValueError):
        ops.lpips(a[:, :, :30], b[:, :, :30], wd)                 # a 30-pixel side
    with pytest.raises(ValueError):
        ops.lpips(a, b, wd, roi=(0, 0, 30, 40))
    with pytest.raises(ValueError):
        ops.lpips(a, b, wd, roi=(10, 0, 31, 40))                  # leaves the image
    with pytest.raises(ValueError):
        metrics.lpips(torch.rand(1, 3, 40, 60, device=DEV), torch.rand(1, 3, 40, 60, device=DEV), wd, half="right")   # a 30-wide half
    with pytest.raises(ValueError):
        ops.lpips(torch.rand(1, 1, 40, 40, device=DEV), torch.rand(1, 1, 40, 40, device=DEV), wd)

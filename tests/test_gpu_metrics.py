"""crnerf_image_metrics_f32 (csrc/metrics.hip) and the layers above it on the GPU, against the float64 restatement of the SSIM
definition that tests/test_metrics_host.py carries and pins.

Map accuracy is measured with the reference's own arithmetic as the unit: e_ref = max |restatement in float32 on the CPU -
restatement in float64| is what kornia-style fp32 evaluation (E[x^2] - mu^2) loses on the same inputs, e_hip = max |HIP map -
float64|, and the bar is e_hip <= 2 e_ref (the factor 2: a different summation order where both are dominated by the same
2 s12 + C2 cancellation; the kernel's centred second moments are expected well under it).  Measured e_ref / e_hip per case are
printed (pytest -s) and appended to the file CRNERF_METRICS_PARITY_OUT names, if set (profiles/r8/metrics_parity.txt).

Scalars: the kernel accumulates in double, so ssim_sum / n is the float64 mean of its own fp32 map up to double rounding (bar
2^-23 relative, one fp32 ulp) and sse is the float64 sse of the same fp32 inputs (bar 2^-22 relative).

Shapes: 2x2 (all border), 3x70, one row and one column past one tile and past two tiles (from ops.METRICS_TILE), 24x41 scored
on its right half (odd width: ROI 21 wide from x0 = 20), one 200x300."""
import os

import pytest
import torch

import crnerf_amd.synth as synth
from crnerf_amd import metrics, ops, pipeline
from oracle import cpu_ref as O
from test_metrics_host import C1, C2, EPS, ssim_restatement

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T = torch.from_numpy
TH, TW = ops.METRICS_TILE
SHAPES = [(2, 2), (3, 70), (TH + 1, TW + 1), (2 * TH + 1, 2 * TW + 1), (24, 41), (200, 300)]
CONTENTS = ["noise", "sinusoid", "flat", "noisy"]


def record(line):
    print(line, flush=True)
    path = os.environ.get("CRNERF_METRICS_PARITY_OUT")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def make_pair(kind, H, W):
    """(pred, gt), (1,3,H,W) float32 on the CPU, seeded by kind and shape."""
    g = torch.Generator().manual_seed(1000 * H + W + 7 * CONTENTS.index(kind))
    if kind == "noise":                                     # two independent uniform images
        return torch.rand(1, 3, H, W, generator=g), torch.rand(1, 3, H, W, generator=g)
    if kind == "sinusoid":
        y, x = torch.arange(H, dtype=torch.float32)[:, None], torch.arange(W, dtype=torch.float32)[None, :]
        c = torch.arange(3, dtype=torch.float32)[:, None, None]
        gt = (0.5 + 0.4 * torch.sin(0.11 * x + 0.07 * y + c))[None].contiguous()
    elif kind == "flat":
        gt = torch.full((1, 3, H, W), 0.7)
    else:
        gt = torch.rand(1, 3, H, W, generator=g)
    return (gt + 0.05 * torch.randn(1, 3, H, W, generator=g)).clamp(0, 1), gt


_cache = {}


def case(kind, H, W):
    """Inputs and float64 / float32 references of one case, computed once and shared (never modified)."""
    key = (kind, H, W)
    if key not in _cache:
        pred, gt = make_pair(kind, H, W)
        half = (H, W) == (24, 41)
        x0 = W // 2 if half else 0
        p, g = pred[..., x0:], gt[..., x0:]                     # the reference crops first and filters afterwards
        r64 = ssim_restatement(p, g, torch.float64)
        e_ref = float((ssim_restatement(p, g, torch.float32).double() - r64).abs().max())
        _cache[key] = dict(pred=pred, gt=gt, half="right" if half else None, roi=(x0, 0, W - x0, H) if half else None, r64=r64, e_ref=e_ref,
                           sse64=float(((p.double() - g.double()) ** 2).sum()), crop=(p, g))
    return _cache[key]


@pytest.mark.parametrize("H,W", SHAPES)
@pytest.mark.parametrize("kind", CONTENTS)
def test_map_and_scalars(kind, H, W):
    c = case(kind, H, W)
    pred, gt = c["pred"].to(DEV), c["gt"].to(DEV)
    sse, ssim_sum, n, m = ops.image_metrics(pred, gt, roi=c["roi"], want_map=True)
    p, g = c["crop"]
    assert n == p.numel() and m.shape == p.shape[1:] and m.dtype == torch.float32 and sse.dtype == torch.float64
    m64 = m.cpu().double()
    e_hip = float((m64 - c["r64"][0]).abs().max())
    record("%-8s %3dx%-3d roi=%s  e_ref %.3e  e_hip %.3e  ratio %.4f" % (kind, H, W, c["roi"], c["e_ref"], e_hip, e_hip / c["e_ref"]))
    assert e_hip <= 2 * c["e_ref"]
    mean = float(m64.mean())
    assert abs(float(ssim_sum) / n - mean) <= 2.0 ** -23 * abs(mean)
    assert abs(float(sse) - c["sse64"]) <= 2.0 ** -22 * c["sse64"]
    assert abs(-10.0 * torch.log10(sse / n).item() - O.psnr(p, g)) <= 1e-4
    # the same call again: the same bits
    sse2, ssim_sum2, _, m2 = ops.image_metrics(pred, gt, roi=c["roi"], want_map=True)
    assert torch.equal(sse, sse2) and torch.equal(ssim_sum, ssim_sum2) and torch.equal(m, m2)
    # the mirror's functions are that launch
    d = metrics.image_metrics(pred, gt, half=c["half"])
    assert torch.equal(d["mse"], (sse / n).float()) and torch.equal(d["ssim"], (ssim_sum / n).float())
    assert torch.equal(d["psnr"], (-10.0 * torch.log10(sse / n)).float()) and d["psnr"].dim() == 0 and d["psnr"].is_cuda
    if c["roi"] is None:
        assert torch.equal(metrics.ssim(pred, gt), m[None]) and metrics.ssim(pred, gt, "sum").shape == (1, 3, H, W)
        assert torch.equal(metrics.mse(pred, gt), d["mse"]) and torch.equal(metrics.psnr(pred, gt), d["psnr"])


@pytest.mark.parametrize("H,W", SHAPES)
def test_layouts_are_read_in_place(H, W):
    """Pixel-major memory seen as CHW (decode_image's [H*W,3] through eval_metric.py's view / permute), and a column slice of a wider
    image: the same bits as the contiguous (1,3,H,W) copy."""
    c = case("noisy", H, W)
    pred, gt = c["pred"].to(DEV), c["gt"].to(DEV)
    want = ops.image_metrics(pred, gt, roi=c["roi"], want_map=True)
    pm = lambda t: t[0].permute(1, 2, 0).reshape(H * W, 3).contiguous().view(H, W, 3).permute(2, 0, 1)[None]  # noqa: E731
    assert pm(pred).stride()[1:] == (1, 3 * W, 3) and not pm(pred).is_contiguous()
    wide_p, wide_g = torch.rand(1, 3, H + 3, W + 9, device=DEV), torch.rand(1, 3, H + 3, W + 9, device=DEV)
    wide_p[..., 2:2 + H, 5:5 + W], wide_g[..., 2:2 + H, 5:5 + W] = pred, gt
    sl_p, sl_g = wide_p[..., 2:2 + H, 5:5 + W], wide_g[..., 2:2 + H, 5:5 + W]
    assert not sl_p.is_contiguous() and torch.equal(sl_p.contiguous(), pred)
    for a, b in ((pm(pred), pm(gt)), (pm(pred), gt), (sl_p, sl_g), (sl_p[0], pm(gt)[0])):
        got = ops.image_metrics(a, b, roi=c["roi"], want_map=True)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and got[2] == want[2] and torch.equal(got[3], want[3])
    # planar [3, H*W] memory behind an [H*W,3] view -- what decode_image hands over -- through the same view
    planar = pred[0].reshape(3, H * W).t()
    got = ops.image_metrics(planar.view(H, W, 3).permute(2, 0, 1)[None], gt, roi=c["roi"], want_map=True)
    assert torch.equal(got[0], want[0]) and torch.equal(got[3], want[3])


@pytest.mark.parametrize("H,W", [(24, 41), (2 * TH + 1, 2 * TW + 1), (2, 5)])
def test_right_half_is_the_cropped_image(H, W):
    pred, gt = (t.to(DEV) for t in make_pair("noisy", H, W))
    crop = lambda t: t[..., W // 2:].contiguous()  # noqa: E731
    a, b = metrics.image_metrics(pred, gt, half="right"), metrics.image_metrics(crop(pred), crop(gt))
    assert all(torch.equal(a[k], b[k]) for k in ("mse", "psnr", "ssim"))
    ra = ops.image_metrics(pred, gt, roi=(W // 2, 0, W - W // 2, H), want_map=True)
    rb = ops.image_metrics(crop(pred), crop(gt), want_map=True)
    assert torch.equal(ra[0], rb[0]) and torch.equal(ra[1], rb[1]) and ra[2] == rb[2] and torch.equal(ra[3], rb[3])
    # a region that starts below the top row too
    if H > 4:
        rc = ops.image_metrics(pred, gt, roi=(3, 2, W - 4, H - 3), want_map=True)
        rd = ops.image_metrics(pred[..., 2:H - 1, 3:W - 1].contiguous(), gt[..., 2:H - 1, 3:W - 1].contiguous(), want_map=True)
        assert torch.equal(rc[0], rd[0]) and torch.equal(rc[1], rd[1]) and torch.equal(rc[3], rd[3])


@pytest.mark.parametrize("H,W", [(TH + 1, TW + 1), (24, 41)])
def test_quantize_pred_is_the_uint8_round_trip(H, W):
    """The PNG round trip of eval.py:296-297 / eval_metric.py:75-76 as the reference makes it -- on the host, where torch's / 255 is a
    true division -- against the kernel's on-load quantisation of the raw prediction (values below 0 and above 1 included)."""
    g = torch.Generator().manual_seed(5)
    gt = torch.rand(1, 3, H, W, generator=g)
    raw = gt + 0.3 * torch.randn(1, 3, H, W, generator=g)
    assert float(raw.min()) < 0 and float(raw.max()) > 1
    png = (raw.clamp(0, 1) * 255).to(torch.uint8).float() / 255
    roi = (W // 2, 0, W - W // 2, H)
    a = ops.image_metrics(raw.to(DEV), gt.to(DEV), roi=roi, quantize_pred=True, want_map=True)
    b = ops.image_metrics(png.to(DEV), gt.to(DEV), roi=roi, quantize_pred=False, want_map=True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[3], b[3])
    c = ops.image_metrics(raw.to(DEV), gt.to(DEV), roi=roi, want_map=True)
    assert not torch.equal(a[0], c[0])
    d, e = metrics.image_metrics(raw.to(DEV), gt.to(DEV), half="right", quantize_pred=True), metrics.image_metrics(png.to(DEV), gt.to(DEV), half="right")
    assert all(torch.equal(d[k], e[k]) for k in d)


def test_constant_and_identical_images():
    """The analytic values of the definition: constant images a, b -> (2ab + C1) C2 / ((a^2 + b^2 + C1) C2 + eps) everywhere; identical
    images -> den / (den + eps), which is 1 - 1e-9 or closer: fp32's 1."""
    for a, b in ((0.7, 0.7), (0.2, 0.9), (0.0, 1.0)):
        pa, pb = torch.full((1, 3, TH + 3, TW + 5), a, device=DEV), torch.full((1, 3, TH + 3, TW + 5), b, device=DEV)
        af, bf = float(pa[0, 0, 0, 0]), float(pb[0, 0, 0, 0])
        want = (2 * af * bf + C1) * C2 / ((af * af + bf * bf + C1) * C2 + EPS)
        m = metrics.ssim(pa, pb)
        assert float((m.double() - want).abs().max()) <= 4 * 2.0 ** -24 * max(want, 2.0 ** -10)
        d = metrics.image_metrics(pa, pb)
        assert abs(float(d["mse"]) - (af - bf) ** 2) <= 2.0 ** -23 * (af - bf) ** 2
    img = torch.rand(1, 3, 2 * TH + 1, TW + 1, device=DEV)
    assert float((metrics.ssim(img, img) - 1).abs().max()) <= 2.0 ** -24
    assert float(metrics.image_metrics(img, img)["mse"]) == 0.0


def test_wrapper_rejects_what_the_kernel_cannot_read():
    a = torch.rand(1, 3, 8, 8, device=DEV)
    for roi in ((0, 0, 1, 8), (0, 0, 8, 1), (1, 0, 8, 8), (0, -1, 8, 8), (0, 0, 0, 0)):
        with pytest.raises(ValueError):
            ops.image_metrics(a, a, roi=roi)
    with pytest.raises(ValueError):
        ops.image_metrics(a, a[..., :7])
    with pytest.raises(TypeError):
        ops.image_metrics(a.double(), a.double())
    with pytest.raises(ValueError):
        metrics.mse(torch.rand(8, device=DEV), torch.rand(8, device=DEV))
    # what the reference's callers hand to psnr: [R,3] rows (train_mask_grid_sample.py:396) and (H,W,3) slices (eval_metric.py:90)
    p, g = torch.rand(64, 3, device=DEV), torch.rand(64, 3, device=DEV)
    assert abs(float(metrics.psnr(p, g)) - O.psnr(p.cpu(), g.cpu())) <= 1e-4
    p, g = torch.rand(8, 9, 3, device=DEV), torch.rand(8, 9, 3, device=DEV)
    assert abs(float(metrics.psnr(p[:, 4:], g[:, 4:])) - O.psnr(p[:, 4:].cpu(), g[:, 4:].cpu())) <= 1e-4


# ------------------------------------------------------------------ orchestration: evaluate_image, validation_step(ssim=True)
class HP:
    maskrs_max, maskrs_min, maskrs_k, maskrd = 5e-2, 6e-3, 1e-3, 1e-3
    weightKL, weightRecA, weightcontent, mse_on_appearance = 1e-5, 1e-3, 1e-4, False
    nerf_out_dim, pertubeCord, N_emb_xyz, N_emb_dir, use_disp, encode_a, encode_random, N_a = 64, False, 15, 4, False, True, True, 48
    img_wh, N_samples, N_importance, perturb, noise_std, chunk, N_vocab = [40, 24], 32, 32, 1.0, 1.0, 2048, 8
    encode_c, use_mask = True, False


def _system():
    """The synthetic system of tests/test_gpu_fullsize.py::test_validation_step_val_mode."""
    torch.manual_seed(0)
    sysm = pipeline.TrainingSystem(HP(), device=DEV)
    sysm.models["coarse"].load_state_dict({k: T(v) for k, v in synth.mlp_state(1, 2.0, 0.5).items()})
    sysm.models["fine"].load_state_dict({k: T(v) for k, v in synth.mlp_state(2, 2.0, 0.5).items()})
    sysm.models["decoder"].load_state_dict({k: T(v) for k, v in synth.decoder_state(3).items()})
    sysm.enc_a.load_state_dict({k: T(v) for k, v in synth.encoder_state(4, 2.0).items()})
    sysm.enc_cont.load_state_dict({k: T(v) for k, v in synth.encoder_state(5, 2.0).items()})
    return sysm


def test_evaluate_image():
    Wd, Ht = 40, 24
    R = Wd * Ht
    sysm = _system()
    sysm.eval()
    hp = sysm.hparams_
    g = torch.Generator().manual_seed(3)
    # one sample as PhototourismDataset(split='test_test') returns it: host tensors, no batch dimension
    sample = {"rays": T(synth.rays(R, H=Ht, W=Wd)), "ts": torch.full((R,), 5, dtype=torch.int64), "rgbs": torch.rand(R, 3, generator=g),
              "whole_img": torch.rand(3, Ht, Wd, generator=g) * 2 - 1, "img_wh": torch.tensor([Wd, Ht])}
    out = pipeline.evaluate_image(sysm.models, sysm.embeddings, sysm.enc_a, sample, hp, chunk=512)
    assert sorted(out) == ["mse", "psnr", "rgb", "ssim"]
    with torch.no_grad():
        a_emb = sysm.enc_a((sample["whole_img"].to(DEV)[None] + 1) / 2)
        res = pipeline.batched_inference(sysm.models, sysm.embeddings, sample["rays"].to(DEV), sample["ts"].to(DEV), hp.N_samples, hp.N_importance,
                                         hp.use_disp, 512, False, args=hp, a_embedded_from_img=a_emb)
        rgb = pipeline.decode_image(sysm.models, res, Ht, Wd, a_emb)
    assert out["rgb"].shape == (R, 3) and torch.equal(out["rgb"], rgb)
    chw = lambda t: t.view(Ht, Wd, 3).permute(2, 0, 1)[None]  # noqa: E731
    want = metrics.image_metrics(chw(rgb), chw(sample["rgbs"].to(DEV)), half="right", quantize_pred=True)
    assert all(torch.equal(out[k], want[k]) and out[k].dim() == 0 and out[k].is_cuda for k in ("mse", "psnr", "ssim"))
    # the reference's protocol on the host: PNG round trip, right half, metrics.psnr / mean of the float64 SSIM map
    png = (rgb.cpu().view(Ht, Wd, 3).clamp(0, 1) * 255).to(torch.uint8).float() / 255
    gt = sample["rgbs"].view(Ht, Wd, 3)
    assert abs(float(out["psnr"]) - O.psnr(gt[:, Wd // 2:], png[:, Wd // 2:])) <= 1e-4
    r64 = ssim_restatement(gt[:, Wd // 2:].permute(2, 0, 1)[None], png[:, Wd // 2:].permute(2, 0, 1)[None])
    r32 = ssim_restatement(gt[:, Wd // 2:].permute(2, 0, 1)[None], png[:, Wd // 2:].permute(2, 0, 1)[None], torch.float32)
    assert abs(float(out["ssim"]) - float(r64.mean())) <= 2 * float((r32.double() - r64).abs().max())
    # raw decode on the whole image: another number
    raw = pipeline.evaluate_image(sysm.models, sysm.embeddings, sysm.enc_a, sample, hp, chunk=512, half=None, quantize_pred=False)
    assert torch.equal(raw["rgb"], rgb) and not torch.equal(raw["mse"], out["mse"])


def test_validation_step_ssim():
    Wd, Ht = 40, 24
    R = Wd * Ht
    sysm = _system()
    batch = {"rays": T(synth.rays(R, H=Ht, W=Wd)).to(DEV)[None], "ts": torch.full((1, R), 5, dtype=torch.int64, device=DEV),
             "rgbs": torch.rand(1, R, 3, device=DEV), "whole_img": torch.rand(1, 3, Ht, Wd, device=DEV) * 2 - 1,
             "img_wh": torch.tensor([[Wd, Ht]]), "rgb_idx": None}
    want = ["val_loss", "kl_a", "rec_a_random", "c_l", "content_constraint", "f_l", "val_psnr"]
    log = sysm.validation_step(batch, 0, ssim=True)
    assert list(log) == want + ["val_ssim", "results"]
    m = log["val_ssim"]
    assert m.shape == (1, 3, Ht, Wd) and m.is_cuda
    chw = lambda t: t.cpu().view(Ht, Wd, 3).permute(2, 0, 1)[None]  # noqa: E731
    pred, gt = chw(log["results"]["rgb_fine"]), chw(batch["rgbs"][0])
    r64 = ssim_restatement(pred, gt)
    e_ref = float((ssim_restatement(pred, gt, torch.float32).double() - r64).abs().max())
    e_hip = float((m.cpu().double() - r64).abs().max())
    record("val_ssim 24x40  e_ref %.3e  e_hip %.3e" % (e_ref, e_hip))
    assert e_hip <= 2 * e_ref
    assert list(sysm.validation_step(batch, 0)) == want + ["results"]

"""precision="bf16_fc" (fp16 coarse pass + bf16 fine pass) on the two trained checkpoints, next to "bf16" and "bf16_hc" in the same run, against the
reference's fp32 outputs through each checkpoint's own trained decoder -- the shape of
tests/test_gpu_trained_ckpt.py::test_trained_checkpoint_bf16_with_fp32_accurate_coarse_pass.  Bars: SURVEY 8d's pixels max-abs <= 4e-3 and
north_star's |delta PSNR vs gt| <= 0.05 dB, both as stated; and the reason the mode exists -- its coarse weights are closer to fp32's than bf16's.
The CPU study (profiles/r6/fp16_coarse_pass_study.txt) priced the pixels at 1.61e-3 (g15) and 2.96e-3 (g16).

And one 800 x 800 frame (configs[2]'s shape) through the mode.
"""
import numpy as np
import pytest
import torch

import crnerf_amd.synth as synth
from crnerf_amd import pipeline
from test_gpu_trained_ckpt import DEV, T, _diff, _load, _psnr, record

pytestmark = pytest.mark.gpu
PIXEL_BAR, PSNR_BAR = 4e-3, 0.05


@torch.no_grad()
@pytest.mark.parametrize("fixture", ["g15_trained", "g16_trained"])
def test_trained_checkpoint_bf16_with_fp16_coarse_pass(golden, tmp_path, fixture):
    g = golden(fixture)
    hp, models, emb, enc_a, side = _load(g, tmp_path)
    rays, style_img = T(g["rays"]).to(DEV), (T(g["style_rgbs"]).t().reshape(1, 3, side, side)).contiguous().to(DEV)
    a = enc_a(style_img)
    ref_rgb, gt = T(g["ref__64_128__rgb_fine"]), T(g["gt"])
    m = {}
    for prec in ("bf16", "bf16_fc", "bf16_hc"):
        res = pipeline.batched_inference(models, emb, rays, None, 64, 128, False, 2048, False, args=hp, a_embedded_from_img=a, precision=prec)
        rgb = pipeline.decode_image(models, res, side, side, a)
        mm = {k: _diff(res[k], T(g["ref__64_128__%s" % k])) for k in ("weights_coarse", "feature_coarse", "feature_fine", "weights_fine", "depth_fine")}
        mm["rgb_fine"] = _diff(rgb, ref_rgb)
        mm["delta_psnr_vs_gt_db"] = _psnr(rgb.cpu(), gt) - _psnr(ref_rgb, gt)
        mm["psnr_vs_reference_db"] = _psnr(rgb.cpu(), ref_rgb)
        m[prec] = mm
    fc = m["bf16_fc"]
    fc["pixel_bar_margin"] = PIXEL_BAR / fc["rgb_fine"]["max_abs"]
    record("%sbf16 vs bf16_fc vs bf16_hc 64_128" % ("" if fixture == "g15_trained" else "g16 "), m)
    for prec in m:
        print("%s %-8s pixels max-abs %.3e  weights_coarse max-abs %.3e  weights_fine rel-L2 %.3e  dPSNR vs gt %+.4f dB" % (
            fixture, prec, m[prec]["rgb_fine"]["max_abs"], m[prec]["weights_coarse"]["max_abs"], m[prec]["weights_fine"]["rel_l2"], m[prec]["delta_psnr_vs_gt_db"]))
    print("%s bf16_fc: %.2fx under the 4e-3 pixel bar" % (fixture, fc["pixel_bar_margin"]))
    assert fc["weights_coarse"]["max_abs"] < m["bf16"]["weights_coarse"]["max_abs"], m      # what the mode is for
    assert abs(fc["delta_psnr_vs_gt_db"]) <= PSNR_BAR, fc
    assert fc["rgb_fine"]["max_abs"] <= PIXEL_BAR, (fc["rgb_fine"], m["bf16"]["rgb_fine"], m["bf16_hc"]["rgb_fine"])


@torch.no_grad()
def test_full_image_bf16_fc_800x800():
    from crnerf_amd.datasets.ray_utils import generate_rays

    class HP:
        nerf_out_dim, pertubeCord, N_emb_xyz, N_emb_dir, use_disp, encode_a, encode_random, N_a = 64, False, 15, 4, False, True, True, 48
        img_wh, N_samples, N_importance = [800, 800], 64, 128
    hp = HP()
    Wd = Ht = 800
    R = Wd * Ht
    models, emb = pipeline.get_model(hp, DEV), pipeline.get_embeddings(hp)
    enc = pipeline.encoder_sameoutputsize(64).to(DEV)
    models["coarse"].load_state_dict({k: T(v) for k, v in synth.mlp_state(1, 3.0, 1.0).items()})
    models["fine"].load_state_dict({k: T(v) for k, v in synth.mlp_state(2, 3.0, 1.0).items()})
    models["decoder"].load_state_dict({k: T(v) for k, v in synth.decoder_state(3).items()})
    enc.load_state_dict({k: T(v) for k, v in synth.encoder_state(4, 2.0).items()})
    focal = Wd / 2 / np.tan(np.pi / 6)
    K = np.array([[focal, 0, Wd / 2], [0, focal, Ht / 2], [0, 0, 1]])
    c2w = np.array([[1, 0, 0, 0.05], [0, -1, 0, 0.02], [0, 0, -1, 0.1]], dtype=np.float32)
    rays = generate_rays(Ht, Wd, K, c2w, 0.0, 5.0, device=torch.device(DEV))
    a_emb = enc(torch.rand(1, 3, 100, 100, generator=torch.Generator().manual_seed(0)).to(DEV))
    img = {}
    for prec in ("bf16_hc", "bf16_fc", "bf16"):
        res = pipeline.batched_inference(models, emb, rays, None, 64, 128, False, 32768, False, args=hp, a_embedded_from_img=a_emb, precision=prec)
        img[prec] = pipeline.decode_image(models, res, Ht, Wd, a_emb)
        if prec == "bf16_fc":
            for k, v in res.items():
                assert torch.isfinite(v).all(), k
            assert res["weights_fine"].shape == (R, 192) and img[prec].shape == (R, 3)
            s = res["weights_fine"].sum(-1)
            assert float(s.max()) <= 1 + 1e-5 and float(res["weights_fine"].min()) >= 0
            assert 0 <= float(img[prec].min()) and float(img[prec].max()) <= 1
    p_fc, p_bf = _psnr(img["bf16_fc"].cpu(), img["bf16_hc"].cpu()), _psnr(img["bf16"].cpu(), img["bf16_hc"].cpu())
    print("800x800: PSNR against the bf16_hc frame: bf16_fc %.2f dB, bf16 %.2f dB" % (p_fc, p_bf))
    assert p_fc > p_bf, (p_fc, p_bf)

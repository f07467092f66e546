"""crnerf_lanczos_resize_u8 (csrc/imageprep.hip) and the builders of crnerf_amd.datasets.images on the GPU.  Every comparison is
torch.equal: against Pillow's stored output (tests/golden/g17_lanczos.npz) where a case is in the fixture, otherwise against the numpy
restatement that tests/test_lanczos_host.py pins to Pillow.  There is no tolerance in this file.

Shapes: the table of tests/_lanczos_cases.py (windows clipped at both ends, ksize nearly the input, odd halves, the 1/8 ratio, each pass
alone, neither pass, an upscale), output sizes one past one and past two tiles of the horizontal pass (ops.LANCZOS_TILE) and row lengths
two bytes past one and one byte past two blocks of the vertical pass (ops.LANCZOS_VBLOCK; 3 w = 257 has no solution), one 700x1000 photo."""
import numpy as np
import pytest
import torch

import _lanczos_cases as L
import crnerf_amd.synth as synth
from crnerf_amd import ops, pipeline
from crnerf_amd.datasets import images
from crnerf_amd.datasets.phototourism_mask_grid_sample import GridSampleBatcher
from crnerf_amd.datasets.ray_utils import generate_rays

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T = torch.from_numpy
TH, TW = ops.LANCZOS_TILE
VB = ops.LANCZOS_VBLOCK
# (H, W, w, h): the horizontal tile one past one / two tiles in both directions (its rows are SOURCE rows), the vertical block likewise
TILE_SHAPES = [(TH + 1, 2 * (TW + 1) + 1, TW + 1, 3), (2 * TH + 1, 8 * (2 * TW + 1) + 3, 2 * TW + 1, 2 * TH + 1 - 4),
               (2 * (TH + 1), 200, (VB + 2) // 3, TH + 1), (30, 2 * (2 * VB + 1) // 3 + 1, (2 * VB + 1) // 3, 2 * TH + 1)]

_cache = {}


def to_tensor(u8):
    """torchvision's ToTensor of a uint8 HWC image, from its definition, on the CPU."""
    return u8.permute(2, 0, 1).contiguous().to(torch.float32).div(255)


def normalize(x):
    """torchvision's Normalize(0.5, 0.5), on the CPU."""
    return (x - 0.5) / 0.5


def reference(key, a, w, h):
    """Pillow's output of a case (uint8 [h, w, 3] CPU tensor): from the fixture when it is there, else the restatement; computed once."""
    if key not in _cache:
        if "golden" not in _cache:
            _cache["golden"] = L.load_golden()
        _cache[key] = T(_cache["golden"][key] if key in _cache["golden"] else L.resize(a, (w, h)))
    return _cache[key]


def photo():
    if "photo" not in _cache:
        _cache["photo"] = L.noise(7, *L.PHOTO)
    return _cache["photo"]


def all_cases():
    cases = [(c[0], c) for c in L.golden_cases()]
    for i, (H, W, w, h) in enumerate(TILE_SHAPES):
        cases.append(("tile%d_noise" % i, ("tile%d_noise" % i, "noise", 400 + i, H, W, w, h, 0)))
        cases.append(("tile%d_blocks" % i, ("tile%d_blocks" % i, "blocks", 500 + i, H, W, w, h, L.block_side(H, W, w, h))))
    return cases


@pytest.mark.parametrize("key,case", all_cases(), ids=[k for k, _ in all_cases()])
def test_resize_equals_pillow(key, case):
    _, kind, seed, H, W, w, h, side = case
    a = L.case_input(case)
    got = ops.lanczos_resize(T(a).to(DEV), (w, h))
    assert got.dtype == torch.uint8 and tuple(got.shape) == (h, w, 3)
    assert torch.equal(got.cpu(), reference(key, a, w, h))


@pytest.mark.parametrize("d", [2, 8])
def test_photo(d):
    a = photo()
    w, h = L.PHOTO[1] // d, L.PHOTO[0] // d
    ref = reference("photo/%d" % d, a, w, h)
    src = T(a).to(DEV)
    assert torch.equal(images.resize_lanczos(src, (w, h)).cpu(), ref)
    assert torch.equal(images.resize_lanczos(T(a), (w, h)).cpu(), ref)                       # a host photo is uploaded as it is
    assert torch.equal(ops.lanczos_resize(src, (w, h), out="rows").cpu(), to_tensor(ref).view(3, -1).permute(1, 0))


@pytest.mark.parametrize("name", ["odd_half", "vertical_only", "horizontal_only", "identity", "upscale"])
def test_fused_stores(name):
    """rows / chw / signed chw of the last pass that runs (both, vertical only, horizontal only, neither) are the CPU torch expressions
    applied to the uint8 result, bit for bit."""
    case = next(c for c in L.golden_cases() if c[0] == name + "_blocks")
    _, kind, seed, H, W, w, h, side = case
    a = L.case_input(case)
    ref = reference(case[0], a, w, h)
    src = T(a).to(DEV)
    tt = to_tensor(ref)
    assert torch.equal(ops.lanczos_resize(src, (w, h), out="u8").cpu(), ref)
    assert torch.equal(ops.lanczos_resize(src, (w, h), out="rows").cpu(), tt.view(3, -1).permute(1, 0))
    assert torch.equal(ops.lanczos_resize(src, (w, h), out="chw").cpu(), tt)
    assert torch.equal(ops.lanczos_resize(src, (w, h), out="chw", signed=True).cpu(), normalize(tt))


def test_rows_into_a_slice_leaves_the_rest_alone():
    case = next(c for c in L.golden_cases() if c[0] == "odd_half_noise")
    _, kind, seed, H, W, w, h, side = case
    a = L.case_input(case)
    n = w * h
    buf = torch.full((n + 2 * 37, 3), -7.0, device=DEV)
    out = ops.lanczos_resize(T(a).to(DEV), (w, h), out="rows", dst=buf[37:37 + n])
    assert out.data_ptr() == buf[37:].data_ptr()
    got = buf.cpu()
    assert torch.equal(got[37:37 + n], to_tensor(reference(case[0], a, w, h)).view(3, -1).permute(1, 0))
    assert bool((got[:37] == -7.0).all()) and bool((got[37 + n:] == -7.0).all())


def test_two_sizes_back_to_back_share_the_workspace():
    """No synchronisation between the calls: the second resize reuses (or regrows) the cached workspace behind the first on the stream."""
    c1 = next(c for c in L.golden_cases() if c[0] == "eighth_noise")
    c2 = next(c for c in L.golden_cases() if c[0] == "odd_half_blocks")
    a1, a2 = L.case_input(c1), L.case_input(c2)
    s1, s2 = T(a1).to(DEV), T(a2).to(DEV)
    torch.cuda.synchronize()
    g1 = ops.lanczos_resize(s1, (c1[5], c1[6]))
    g2 = ops.lanczos_resize(s2, (c2[5], c2[6]))
    g3 = ops.lanczos_resize(s1, (c1[5], c1[6]))
    assert torch.equal(g1.cpu(), reference(c1[0], a1, c1[5], c1[6])) and torch.equal(g2.cpu(), reference(c2[0], a2, c2[5], c2[6]))
    assert torch.equal(g3.cpu(), g1.cpu())


def test_validation():
    img = torch.zeros(16, 12, 3, dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError, match="uint8"):
        ops.lanczos_resize(img.float(), (6, 8))
    with pytest.raises(ValueError, match="contiguous"):
        ops.lanczos_resize(torch.zeros(16, 24, 3, dtype=torch.uint8, device=DEV)[:, ::2], (6, 8))
    with pytest.raises(ValueError, match=r"\[H, W, 3\]"):
        ops.lanczos_resize(torch.zeros(16, 12, 4, dtype=torch.uint8, device=DEV), (6, 8))
    with pytest.raises(ValueError, match="dst"):
        ops.lanczos_resize(img, (6, 8), out="rows", dst=torch.empty(48, 3, dtype=torch.float64, device=DEV))
    with pytest.raises(ValueError, match="dst"):
        ops.lanczos_resize(img, (6, 8), out="rows", dst=torch.empty(47, 3, device=DEV))
    with pytest.raises(ValueError, match="dst"):
        ops.lanczos_resize(img, (6, 8), out="rows", dst=torch.empty(48, 6, device=DEV)[:, ::2])
    with pytest.raises(ValueError, match="out must be"):
        ops.lanczos_resize(img, (6, 8), out="rows", signed=True)
    with pytest.raises(ValueError, match="below 1x1"):
        ops.lanczos_resize(img, (0, 8))


# ------------------------------------------------------------------ builders
def _camera(w, h, seed):
    rng = np.random.default_rng(seed)
    K = np.array([[0.9 * w, 0, w / 2], [0, 0.9 * w, h / 2], [0, 0, 1]], dtype=np.float32)
    c2w = np.concatenate([np.linalg.qr(rng.normal(size=(3, 3)))[0], rng.normal(size=(3, 1))], 1).astype(np.float32)
    return K, torch.from_numpy(c2w)


def _photo_70x131():
    case = next(c for c in L.golden_cases() if c[0] == "blocky_half_noise")
    return L.case_input(case)                                   # 70 x 131


def test_make_eval_sample():
    a = _photo_70x131()
    H, W = a.shape[:2]
    w, h = W // 2, H // 2
    K, c2w = _camera(w, h, 1)
    s = images.make_eval_sample(T(a), K, c2w, 0.3, 4.5, 17, img_downscale=2)
    assert sorted(s) == ["c2w", "img_wh", "rays", "rgb_idx", "rgbs", "ts", "whole_img"]
    assert s["c2w"] is c2w
    assert {k: (tuple(v.shape), v.dtype) for k, v in s.items() if k != "c2w"} == {
        "rgbs": ((h * w, 3), torch.float32), "rays": ((h * w, 8), torch.float32), "ts": ((h * w,), torch.int64),
        "img_wh": ((2,), torch.int64), "rgb_idx": ((h * w,), torch.int64), "whole_img": ((3, H // 8, W // 8), torch.float32)}
    assert s["img_wh"].tolist() == [w, h] and not s["img_wh"].is_cuda
    assert all(s[k].is_cuda for k in ("rgbs", "rays", "ts", "rgb_idx", "whole_img"))
    assert torch.equal(s["rgbs"].cpu(), to_tensor(reference("blocky_half_noise", a, w, h)).view(3, -1).permute(1, 0))
    assert torch.equal(s["whole_img"].cpu(), normalize(to_tensor(T(L.resize(a, (W // 8, H // 8))))))
    assert torch.equal(s["rays"], generate_rays(h, w, K, c2w, 0.3, 4.5, device=DEV))
    assert torch.equal(s["ts"].cpu(), torch.full((h * w,), 17, dtype=torch.int64)) and torch.equal(s["rgb_idx"].cpu(), torch.arange(h * w))
    # img_downscale 1: no resize runs, rgbs is ToTensor of the photo itself
    K1, _ = _camera(W, H, 1)
    s1 = images.make_eval_sample(T(a).to(DEV), K1, c2w, 0.3, 4.5, 17, img_downscale=1)
    assert s1["img_wh"].tolist() == [W, H]
    assert torch.equal(s1["rgbs"].cpu(), to_tensor(T(a)).view(3, -1).permute(1, 0))
    assert torch.equal(s1["whole_img"], s["whole_img"])


def test_style_image():
    a = _photo_70x131()
    H, W = a.shape[:2]
    tt = to_tensor(T(L.resize(a, (W // 8, H // 8))))
    assert torch.equal(images.style_image(T(a)).cpu(), tt[None])
    assert torch.equal(images.style_image(T(a), signed=True).cpu(), normalize(tt)[None])
    assert torch.equal(images.style_image(T(a), downscale=2).cpu(), to_tensor(reference("blocky_half_noise", a, W // 2, H // 2))[None])


def test_build_train_buffers():
    photos = [L.noise(31, 40, 52), L.blocks(32, 37, 70, 6), L.noise(33, 64, 33)]
    ids = [4, 11, 7]
    cams = [_camera(p.shape[1] // 2, p.shape[0] // 2, 40 + i) for i, p in enumerate(photos)]
    nears, fars = [0.1, 0.2, 0.3], [4.0, 4.5, 5.0]
    # an iterator, one host photo and two device photos
    imgs = iter([T(photos[0]), T(photos[1]).to(DEV), T(photos[2]).to(DEV)])
    all_rays, all_rgbs, all_imgs_wh, all_imgs = images.build_train_buffers(imgs, [c[0] for c in cams], [c[1] for c in cams], nears, fars, ids, 2)
    sizes = [(p.shape[1] // 2, p.shape[0] // 2) for p in photos]
    N = sum(w * h for w, h in sizes)
    assert tuple(all_rays.shape) == (N, 9) and tuple(all_rgbs.shape) == (N, 3) and all_rays.is_cuda and all_rgbs.is_cuda
    assert all_imgs_wh.tolist() == [[float(w), float(h)] for w, h in sizes]
    batcher = GridSampleBatcher(all_rays, all_rgbs, all_imgs_wh, batch_size=64, all_imgs=all_imgs)
    assert batcher._offsets.tolist() == [0] + list(np.cumsum([w * h for w, h in sizes]))
    assert batcher._image_ids == ids
    for i, p in enumerate(photos):
        lo, hi = int(batcher._offsets[i]), int(batcher._offsets[i + 1])
        w, h = sizes[i]
        assert torch.equal(all_rgbs[lo:hi].cpu(), to_tensor(T(L.resize(p, (w, h)))).view(3, -1).permute(1, 0))
        assert torch.equal(all_rays[lo:hi, :8], generate_rays(h, w, cams[i][0], cams[i][1], nears[i], fars[i], device=DEV))
        assert bool((all_rays[lo:hi, 8] == float(ids[i])).all())
        H, W = p.shape[:2]                                        # the appearance image: // 8 of the ORIGINAL photo
        assert torch.equal(all_imgs[i].cpu(), normalize(to_tensor(T(L.resize(p, (W // 8, H // 8))))))
    s = batcher[0]
    assert tuple(s["rays"].shape) == (64, 8) and tuple(s["rgbs"].shape) == (64, 3) and s["image_id"] in ids
    assert s["whole_img"] is all_imgs[ids.index(s["image_id"])]


class HP:
    maskrs_max, maskrs_min, maskrs_k, maskrd = 5e-2, 6e-3, 1e-3, 1e-3
    weightKL, weightRecA, weightcontent, mse_on_appearance = 1e-5, 1e-3, 1e-4, False
    nerf_out_dim, pertubeCord, N_emb_xyz, N_emb_dir, use_disp, encode_a, encode_random, N_a = 64, False, 15, 4, False, True, True, 48
    img_wh, N_samples, N_importance, perturb, noise_std, chunk, N_vocab = [65, 35], 16, 16, 1.0, 1.0, 2048, 32
    encode_c, use_mask = True, False


def test_sample_feeds_evaluate_image():
    """Plumbing only: a decoded photo plus its camera goes through make_eval_sample -> evaluate_image and comes back with finite scores."""
    torch.manual_seed(0)
    sysm = pipeline.TrainingSystem(HP(), device=DEV)
    sysm.models["coarse"].load_state_dict({k: T(v) for k, v in synth.mlp_state(1, 2.0, 0.5).items()})
    sysm.models["fine"].load_state_dict({k: T(v) for k, v in synth.mlp_state(2, 2.0, 0.5).items()})
    sysm.models["decoder"].load_state_dict({k: T(v) for k, v in synth.decoder_state(3).items()})
    sysm.enc_a.load_state_dict({k: T(v) for k, v in synth.encoder_state(4, 2.0).items()})
    sysm.eval()
    a = _photo_70x131()
    K, c2w = _camera(65, 35, 2)
    sample = images.make_eval_sample(T(a), K, c2w, 0.5, 4.0, 5, img_downscale=2)
    out = pipeline.evaluate_image(sysm.models, sysm.embeddings, sysm.enc_a, sample, sysm.hparams_, chunk=1024)
    assert tuple(out["rgb"].shape) == (35 * 65, 3)
    for k in ("psnr", "ssim", "mse"):
        assert bool(torch.isfinite(out[k])), k

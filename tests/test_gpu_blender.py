"""crnerf_rgba_prepare_u8 (csrc/rgbaprep.hip), crnerf_grid_sample_batch_round_f32 and crnerf_amd.datasets.blender on the GPU.  Every
comparison is torch.equal / np.array_equal: against Pillow's and the reference's recorded outputs (tests/golden/g19_blender.npz) where a
case is in the fixture, otherwise against the numpy restatement that tests/test_blender_host.py pins to Pillow.  No tolerance in this file.

Shapes: the table of tests/_lanczos_cases.py on three alpha patterns, output sizes one past one and past two tiles of the horizontal pass
(ops.RGBA_TILE) in both directions, row lengths one pixel past one and past two blocks of the vertical pass (ops.RGBA_VBLOCK), a 24 x 31
frame for the occluders, the reference's three 640 x 640 frames at 40 x 40, one 800 x 800 frame."""
import numpy as np
import pytest
import torch

import _blender_cases as B
from crnerf_amd import ops
from crnerf_amd.datasets import blender
from crnerf_amd.datasets.phototourism_mask_grid_sample import GridSampleBatcher

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T = torch.from_numpy
TH, TW = ops.RGBA_TILE
VB = ops.RGBA_VBLOCK
# (H, W, w, h): the horizontal tile one past one / two tiles in both directions (its rows are SOURCE rows); the vertical block one pixel
# past one block (that pass alone: it then carries the load stage) and one past two blocks (behind the horizontal pass)
TILE_SHAPES = [(TH + 1, 2 * (TW + 1) + 1, TW + 1, 3), (2 * TH + 1, 8 * (2 * TW + 1) + 3, 2 * TW + 1, 2 * TH + 1 - 4),
               (2 * (TH + 1), VB + 1, VB + 1, TH + 1), (2 * TH + 3, 2 * (2 * VB + 1) + 1, 2 * VB + 1, TH - 1)]
BOTH = ["occ", "color"]

_cache = {}


def golden():
    if "golden" not in _cache:
        z = B.load_golden()
        _cache["golden"] = {k: z[k] for k in z.files}
    return _cache["golden"]


def reference(key, a, w, h):
    """Pillow's output of a case (uint8 [h, w, 4] CPU tensor): from the fixture when it is there, else the restatement; computed once."""
    if key not in _cache:
        g = golden()
        _cache[key] = T(g["out_" + key] if "out_" + key in g else B.resize(a, (w, h)))
    return _cache[key]


def frames():
    if "frames" not in _cache:
        _cache["frames"] = [B.frame(t) for t in range(B.N_FRAMES)]
    return _cache["frames"]


def all_cases():
    cases = [(c[0], c) for c in B.table_cases()]
    for i, (H, W, w, h) in enumerate(TILE_SHAPES):
        for j, pat in enumerate(("noise", "blocks")):
            key = "tile%d_%s" % (i, pat)
            cases.append((key, (key, pat, 2000 + 10 * i + j, H, W, w, h)))
    return cases


@pytest.mark.parametrize("key,case", all_cases(), ids=[k for k, _ in all_cases()])
def test_resize_equals_pillow(key, case):
    _, _, _, H, W, w, h = case
    a = B.case_input(case)
    got = ops.rgba_prepare(T(a).to(DEV), (w, h))
    assert got.dtype == torch.uint8 and tuple(got.shape) == (h, w, 4)
    assert torch.equal(got.cpu(), reference(key, a, w, h))


@pytest.mark.parametrize("name", B.SHARES)
def test_fused_stores(name):
    """rows / chw / signed chw / valid_mask of the last pass that runs (both, vertical only, horizontal only, neither, an upscale) are the
    CPU torch expressions applied to the uint8 result, bit for bit; a dst slice leaves its neighbours alone."""
    case = next(c for c in B.table_cases() if c[0] == name + "_blocks")
    _, _, _, H, W, w, h = case
    a = B.case_input(case)
    ref = reference(case[0], a, w, h)
    want = B.tensors(ref.numpy())
    src = T(a).to(DEV)
    u8, valid = ops.rgba_prepare(src, (w, h), out="u8", valid_mask=True)
    assert torch.equal(u8.cpu(), ref) and valid.dtype == torch.bool and torch.equal(valid.cpu(), want["valid"])
    rows, valid = ops.rgba_prepare(src, (w, h), out="rows", valid_mask=True)
    assert torch.equal(rows.cpu(), want["rows"]) and torch.equal(valid.cpu(), want["valid"])
    assert torch.equal(ops.rgba_prepare(src, (w, h), out="chw").cpu(), want["chw"])
    assert torch.equal(ops.rgba_prepare(src, (w, h), out="chw", signed=True).cpu(), want["signed"])
    n = w * h
    buf = torch.full((n + 2 * 37, 3), -7.0, device=DEV)
    out = ops.rgba_prepare(src, (w, h), out="rows", dst=buf[37:37 + n])
    assert out.data_ptr() == buf[37:].data_ptr()
    got = buf.cpu()
    assert torch.equal(got[37:37 + n], want["rows"])
    assert bool((got[:37] == -7.0).all()) and bool((got[37 + n:] == -7.0).all())
    planes = torch.full((3, 3, h, w), -7.0, device=DEV)
    ops.rgba_prepare(src, (w, h), out="chw", signed=True, dst=planes[1])
    got = planes.cpu()
    assert torch.equal(got[1], want["signed"]) and bool((got[0] == -7.0).all()) and bool((got[2] == -7.0).all())


def test_identity_keeps_translucent_pixels():
    """w == W and h == H: no premultiply round trip -- a kernel that premultiplies anyway changes the colour bytes under alpha 1, 128, 254."""
    case = next(c for c in B.table_cases() if c[0] == "identity_edges")
    a = B.case_input(case)
    got = ops.rgba_prepare(T(a).to(DEV), (case[5], case[6])).cpu()
    assert torch.equal(got, T(a)) and torch.equal(got, reference(case[0], a, case[5], case[6]))
    assert not np.array_equal(B.unpremultiply(B.premultiply(a))[0], a)


OCC_H, OCC_W = 24, 31
OCCLUDERS = {
    "none": [],
    "left": [(-5, 3, 4, 9)], "top": [(6, -2, 12, 3)], "right": [(25, 5, 40, 11)], "bottom": [(3, 20, 9, 30)],
    "outside": [(31, 0, 40, 10)], "outside_above": [(0, -9, 30, -1)],
    "overlap": [(4, 4, 15, 15), (10, 8, 22, 20)],
    "ten": [(1 + 2 * i, 2 + i, 3 + 2 * i, 12 + i) for i in range(10)],          # each overlaps the next by one column, as the reference's
    "pixel": [(7, 11, 7, 11)],
    "sixteen": [(i, i, i + 9, i + 5) for i in range(16)],
}


@pytest.mark.parametrize("with_lut", [False, True], ids=["plain", "lut"])
@pytest.mark.parametrize("name", list(OCCLUDERS))
def test_occluders(name, with_lut):
    a = B.make_input("edges", 77, OCC_H, OCC_W)
    rects = np.array(OCCLUDERS[name], dtype=np.int32).reshape(-1, 4)
    colors = np.random.default_rng(len(rects)).integers(0, 256, (len(rects), 3), dtype=np.uint8)
    lut = B.color_table([1.13, 0.84, 1.19], [-0.11, 0.17, 0.02]) if with_lut else None
    painted = B.perturb(a, rects, colors, lut)
    src = T(a).to(DEV)
    kw = dict(rects=rects, colors=colors, lut=lut)
    assert torch.equal(ops.rgba_prepare(src, (OCC_W, OCC_H), **kw).cpu(), T(painted))                 # the load stage alone
    for size in ((16, 12), (OCC_W, 12), (16, OCC_H)):                                                 # ... in front of both passes, of either
        assert torch.equal(ops.rgba_prepare(src, size, **kw).cpu(), T(B.resize(painted, size))), size
    rows, valid = ops.rgba_prepare(src, (16, 12), out="rows", valid_mask=True, **kw)
    want = B.tensors(B.resize(painted, (16, 12)))
    assert torch.equal(rows.cpu(), want["rows"]) and torch.equal(valid.cpu(), want["valid"])


@pytest.mark.parametrize("seed", B.PERTURB_SEEDS)
def test_add_perturbation_equals_the_references(seed):
    g = golden()
    src = T(frames()[0]).to(DEV)
    for pset in B.PERTURB_SETS:
        full = blender.add_perturbation(src, list(pset), seed)
        assert full.dtype == torch.uint8 and tuple(full.shape) == (B.FRAME, B.FRAME, 4)
        assert torch.equal(ops.rgba_prepare(full, B.IMG_WH).cpu(), T(g["pert_%d_%s" % (seed, "_".join(pset))]))


def build():
    if "buffers" not in _cache:
        _cache["buffers"] = blender.build_train_buffers(frames(), B.poses(), B.CAMERA_ANGLE_X, B.IMG_WH, perturbation=BOTH)
        _cache["np_state"] = np.random.get_state()
    return _cache["buffers"]


def test_build_train_buffers_against_the_reference():
    g = golden()
    all_rays, all_rgbs, all_imgs = build()
    n = B.N_FRAMES * B.IMG_WH[0] * B.IMG_WH[1]
    assert tuple(all_rays.shape) == (n, 9) and tuple(all_rgbs.shape) == (n, 3) and tuple(all_imgs.shape) == (B.N_FRAMES, 3, 40, 40)
    assert all(t.is_cuda and t.dtype == torch.float32 for t in (all_rays, all_rgbs, all_imgs))
    assert torch.equal(all_rgbs.cpu(), T(g["train_all_rgbs"]))
    assert torch.equal(all_imgs.cpu(), T(g["train_all_imgs"]))
    assert torch.equal(all_rays.cpu(), T(g["train_all_rays"]))
    dev_frames = [T(a).to(DEV) for a in frames()]                                                     # a device photo gives the same
    again = blender.build_train_buffers(iter(dev_frames), B.poses(), B.CAMERA_ANGLE_X, B.IMG_WH, perturbation=BOTH)
    assert all(torch.equal(x, y) for x, y in zip(again, (all_rays, all_rgbs, all_imgs)))
    plain = blender.build_train_buffers(frames()[:2], B.poses()[:2], B.CAMERA_ANGLE_X, B.IMG_WH)
    assert torch.equal(plain[1][:1600], all_rgbs[:1600]) and not torch.equal(plain[1][1600:], all_rgbs[1600:3200])


def test_rays_against_the_reference():
    """all_rays of the reference's own dataset, every column: the directions need the fma-accumulated norm of
    crnerf_generate_rays_fmanorm_f32; the default generate_rays differs from it in some values, by a few ulp."""
    from crnerf_amd.datasets.ray_utils import generate_rays
    g = golden()
    assert torch.equal(build()[0].cpu(), T(g["train_all_rays"]))
    K, pose = blender.intrinsics(B.CAMERA_ANGLE_X, 40, 40), B.poses()[1]
    fused, plain = generate_rays(40, 40, K, pose, 2.0, 6.0, device=DEV, fma_norm=True), generate_rays(40, 40, K, pose, 2.0, 6.0, device=DEV)
    assert torch.equal(fused.cpu(), T(g["train_all_rays"])[1600:3200, :8])
    assert not torch.equal(fused, plain)


@pytest.mark.parametrize("idx", [0, 1])
def test_make_eval_sample_against_the_reference(idx):
    g = golden()
    pose = T(B.poses()[idx])
    s = blender.make_eval_sample(frames()[idx], pose, B.CAMERA_ANGLE_X, B.IMG_WH, idx, "test_train", perturbation=BOTH)
    assert sorted(s) == ["c2w", "original_rgbs", "original_valid_mask", "rays", "rgb_idx", "rgbs", "ts", "valid_mask"]
    assert s["c2w"] is pose and s["valid_mask"].dtype == torch.bool and s["ts"].dtype == torch.int64
    for k in ("rays", "ts", "rgbs", "valid_mask", "rgb_idx", "original_rgbs", "original_valid_mask"):
        assert torch.equal(s[k].cpu(), T(g["eval%d_%s" % (idx, k)])), k
    assert torch.equal(s["rays"], build()[0][idx * 1600:(idx + 1) * 1600, :8])
    dev = blender.make_eval_sample(T(frames()[idx]).to(DEV), pose, B.CAMERA_ANGLE_X, B.IMG_WH, idx, "test_train", perturbation=BOTH)
    assert all(torch.equal(dev[k], s[k]) for k in s)
    val = blender.make_eval_sample(frames()[idx], pose, B.CAMERA_ANGLE_X, B.IMG_WH, idx, "val", perturbation=BOTH)
    assert sorted(val) == ["c2w", "rays", "rgb_idx", "rgbs", "ts", "valid_mask"] and int(val["ts"].max()) == 0
    assert torch.equal(val["rgbs"].cpu(), T(g["eval%d_original_rgbs" % idx]))


def test_whole_image_against_the_reference():
    g = golden()
    got = blender.whole_image(frames()[0], B.IMG_WH)
    assert tuple(got.shape) == (1, 3, 40, 40) and torch.equal(got.cpu(), T(g["whole_img"]))
    assert torch.equal(blender.whole_image(T(frames()[0]).to(DEV), B.IMG_WH), got)


def test_batcher_reproduces_the_recorded_samples():
    """The reference's buffers in, the reference's two recorded samples out: the first on the numpy state build_train_buffers leaves behind
    (the reference's constructor leaves the same), the second after np.random.seed; torch seeded as recorded."""
    g = golden()
    build()
    np.random.set_state(_cache["np_state"])
    b = blender.BlenderGridSampleBatcher(T(g["train_all_rays"]).to(DEV), T(g["train_all_rgbs"]).to(DEV), T(g["train_all_imgs"]).to(DEV),
                                         B.IMG_WH, batch_size=64)
    assert len(b) == 3 * 1600 // 64
    for n in (0, 1):
        np_seed, torch_seed, idx = (int(v) for v in g["sample%d_setup" % n])
        if np_seed >= 0:
            np.random.seed(np_seed)
        torch.manual_seed(torch_seed)
        b.scale_anneal = float(g["sample%d_anneal" % n])
        s = b[idx]
        assert s["min_scale_cur"] == float(g["sample%d_min_scale_cur" % n])
        for k in ("rays", "ts", "rgbs", "whole_img", "rgb_idx", "uv_sample"):
            assert np.array_equal(s[k].cpu().numpy(), g["sample%d_%s" % (n, k)]), (n, k)
            assert s[k].dtype == (torch.int64 if k in ("ts", "rgb_idx") else torch.float32)
    with pytest.raises(ValueError, match="2\\^24"):
        blender.BlenderGridSampleBatcher(b.all_rays, b.all_rgbs, None, (4097, 4096))


def gather(k, **kw):
    """One lattice node (lin = 0, scale = 1) of a 64 x 64 image whose row r of all_rays / all_rgbs holds r: h_offset = (k + 0.5) / 64."""
    n = 64 * 64
    rows = torch.arange(n, dtype=torch.float32, device=DEV)
    all_rays = rows[:, None].repeat(1, 9).contiguous()
    lin = torch.zeros(1, device=DEV)
    return ops.grid_sample_batch(all_rays, all_rays[:, :3].contiguous(), 0, 64, 64, 1, lin, lin, 1.0, (k + 0.5) / 64, 5 / 64, **kw)


def test_round_is_half_to_even_and_floor_is_untouched():
    for k, row in ((2, 2), (3, 4)):
        s = gather(k, rounding="round")
        assert int(s["rgb_idx"][0]) == row * 64 + 5 and float(s["rays"][0, 0]) == row * 64 + 5 and int(s["ts"][0]) == row * 64 + 5
        for f in (gather(k, rounding="floor"), gather(k)):
            assert int(f["rgb_idx"][0]) == k * 64 + 5 and float(f["rgbs"][0, 2]) == k * 64 + 5
    with pytest.raises(ValueError, match="rounding"):
        gather(2, rounding="ceil")


@pytest.mark.parametrize("tag", ["a", "b", "c"])
def test_existing_gather_is_unchanged_on_its_own_inputs(golden, tag):
    """tests/test_gpu_train_aux.py's recorded Phototourism samples, through the default call (rounding="floor")."""
    g = golden("g11_batcher")
    v = lambda k: g[tag + "__" + k]  # noqa: E731
    b = GridSampleBatcher(T(g["all_rays"]).to(DEV), T(g["all_rgbs"]).to(DEV), g["wh"], batch_size=int(v("batch")),
                          scale_anneal=float(v("anneal")), min_scale=float(v("min_scale")))
    b.iterations = int(v("iterations"))
    torch.manual_seed(int(v("torch_seed")))
    s = b.__getitem__(int(v("idx")), current_epoch=int(v("epoch")))
    for k in ("rays", "ts", "rgbs", "rgb_idx", "uv_sample"):
        assert np.array_equal(s[k].cpu().numpy(), v(k)), k


def test_full_frame_with_both_perturbations():
    """800 x 800 -> 400 x 400, occluders and colour table, against the restatement; 800 -> 25 (the widest ratio the header promises) runs."""
    a = B.frame(1, side=800)
    rects, colors, lut = blender.perturbation_params(BOTH, 5)
    want = B.resize(B.perturb(a, rects, colors, lut), (400, 400))
    src = T(a).to(DEV)
    got, valid = ops.rgba_prepare(src, (400, 400), rects=rects, colors=colors, lut=lut, valid_mask=True)
    assert torch.equal(got.cpu(), T(want)) and torch.equal(valid.cpu(), T(want[..., 3].reshape(-1) > 0))
    assert torch.equal(ops.rgba_prepare(src, (25, 25)).cpu(), T(B.resize(a, (25, 25))))


def test_validation():
    img = torch.zeros(16, 12, 4, dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError, match="uint8"):
        ops.rgba_prepare(img.float(), (6, 8))
    with pytest.raises(ValueError, match=r"\[H, W, 4\]"):
        ops.rgba_prepare(img[..., :3].contiguous(), (6, 8))
    with pytest.raises(ValueError, match="contiguous"):
        ops.rgba_prepare(img.permute(1, 0, 2), (6, 8))
    with pytest.raises(ValueError, match="GPU tensor"):
        ops.rgba_prepare(img.cpu(), (6, 8))
    with pytest.raises(ValueError, match="signed"):
        ops.rgba_prepare(img, (6, 8), out="rows", signed=True)
    with pytest.raises(ValueError, match="below 1x1"):
        ops.rgba_prepare(img, (0, 8))
    with pytest.raises(ValueError, match="dst"):
        ops.rgba_prepare(img, (6, 8), out="rows", dst=torch.empty(47, 3, device=DEV))
    with pytest.raises(ValueError, match="rectangles"):
        ops.rgba_prepare(img, (6, 8), rects=np.zeros((17, 4)), colors=np.zeros((17, 3)))
    with pytest.raises(ValueError, match="lut"):
        ops.rgba_prepare(img, (6, 8), lut=np.zeros((3, 255), dtype=np.uint8))
    with pytest.raises(RuntimeError, match="x1 < x0"):
        ops.rgba_prepare(img, (6, 8), rects=[(5, 0, 4, 3)], colors=[(1, 2, 3)])

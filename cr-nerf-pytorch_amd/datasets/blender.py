"""The reference's Blender dataset (datasets/blender_mask_grid_sample.py) between the decoded RGBA frame and the renderer, on the device:
add_perturbation (:16-36), Pillow's LANCZOS resize of an RGBA image, ToTensor, the blend on white and Normalize (:106-110, :174-178,
eval.py:99-111), bit for bit (csrc/rgbaprep.hip; include/crnerf_blender.h and DESIGN 3.6 N9 state the arithmetic), and on top of that the
training buffers, the evaluation sample and the grid-sample batcher of BlenderDataset.  A decoded frame (uint8 [H, W, 4]) with its pose and
the scene's camera_angle_x is all the host supplies.  Reading the PNG files and parsing transforms_*.json stay outside.
NeuralRenderer_downsampleto of the reference's constructor is not offered: no recipe of the reference sets it, the rays are built at img_wh.

perturbation_params and intrinsics are host-only (numpy): this module imports without the HIP library."""
from math import exp, sqrt

import numpy as np
import torch

NEAR, FAR = 2.0, 6.0      # bounds, common for all scenes (:84-85)
PERTURBATIONS = ("color", "occ")


def _check_perturbation(perturbation):
    perturbation = [perturbation] if isinstance(perturbation, str) else list(perturbation)
    if not set(perturbation).issubset(PERTURBATIONS):
        raise ValueError('Only "color" and "occ" perturbations are supported! (got %r)' % (perturbation,))
    return perturbation


def perturbation_params(perturbation, seed):
    """What add_perturbation(img, perturbation, seed) (:16-36) draws, as data: (rects int32 [n, 4] = inclusive (x0, y0, x1, y1), colors uint8
    [n, 3], lut uint8 [3, 256] or None).  'occ': n = 10 rectangles, else n = 0; 'color': lut[c][v] = (uint8)(255 * clip(s[c] * (v / 255.0) +
    b[c], 0, 1)) in float64 -- the reference's expression for one byte, alpha passing through it unchanged; else None.
    SIDE EFFECT, kept on purpose: the draws come from numpy's legacy GLOBAL generator with the reference's calls in the reference's order
    (np.random.seed(seed), randint twice; np.random.seed(10 * seed + i), choice, per rectangle; np.random.seed(seed), uniform twice), and the
    global state is left where the reference leaves it -- BlenderDataset.__getitem__ draws sample_ts from that unseeded stream."""
    perturbation = _check_perturbation(perturbation)
    rects, colors, lut = np.zeros((0, 4), dtype=np.int32), np.zeros((0, 3), dtype=np.uint8), None
    if 'occ' in perturbation:
        np.random.seed(seed)
        left = np.random.randint(200, 400)
        top = np.random.randint(200, 400)
        rects, colors = np.zeros((10, 4), dtype=np.int32), np.zeros((10, 3), dtype=np.uint8)
        for i in range(10):
            np.random.seed(10 * seed + i)
            colors[i] = np.random.choice(range(256), 3)
            rects[i] = (left + 20 * i, top, left + 20 * (i + 1), top + 200)
    if 'color' in perturbation:
        np.random.seed(seed)
        s = np.random.uniform(0.8, 1.2, size=3)
        b = np.random.uniform(-0.2, 0.2, size=3)
        v = np.arange(256, dtype=np.float64)[:, None] / 255.0
        lut = np.ascontiguousarray((255 * np.clip(s * v + b, 0, 1)).astype(np.uint8).T)
    return rects, colors, lut


def _device_frame(img_u8, device=None):
    """The frame as a contiguous uint8 [H, W, 4] device tensor (a host tensor / array is uploaded as it is: one copy of the decoded bytes)."""
    t = torch.as_tensor(img_u8)
    if not t.is_cuda:
        t = t.to(device if device is not None else torch.device("cuda", torch.cuda.current_device()))
    return t.contiguous()


def _prepare(img, img_wh, params, **kw):
    """ops.rgba_prepare of a device frame; params: perturbation_params(...) or None for the frame as it is."""
    from .. import ops
    rects, colors, lut = params if params is not None else (None, None, None)
    return ops.rgba_prepare(img, img_wh, rects=rects, colors=colors, lut=lut, **kw)


def add_perturbation(img_u8, perturbation, seed):
    """uint8 [H, W, 4] on the device == np.array(add_perturbation(Image.fromarray(img), perturbation, seed)) of the reference (:16-36)."""
    img = _device_frame(img_u8)
    return _prepare(img, (int(img.shape[1]), int(img.shape[0])), perturbation_params(perturbation, seed), out="u8")


def intrinsics(camera_angle_x, w, h):
    """float64 K [3, 3] of read_meta (:74-81): focal = 0.5 * 800 / tan(0.5 * camera_angle_x) * (w / 800), principal point (w / 2, h / 2)."""
    focal = 0.5 * 800 / np.tan(0.5 * camera_angle_x)
    focal *= w / 800
    K = np.eye(3)
    K[0, 0] = K[1, 1] = focal
    K[0, 2] = w / 2
    K[1, 2] = h / 2
    return K


def whole_image(img_u8, img_wh):
    """[1, 3, h, w] in [-1, 1]: eval.py:99-111 -- the frame resized to img_wh, ToTensor, blended on white, Normalize(0.5, 0.5)."""
    w, h = (int(v) for v in img_wh)
    return _prepare(_device_frame(img_u8), (w, h), None, out="chw", signed=True)[None]


def build_train_buffers(images, c2ws, camera_angle_x, img_wh, perturbation=()):
    """The training buffers of BlenderDataset(split='train') (:92-124) on the device: (all_rays [N, 9], all_rgbs [N, 3], all_imgs
    [n, 3, h, w] in [-1, 1]), N = n * h * w, ready for BlenderGridSampleBatcher.  images: decoded frames, uint8 [H, W, 4], on the host or the
    device, in the order of transforms_train.json; they go through the device one at a time.  Frame t is perturbed with seed t unless t == 0
    (:102-104).  Rays: generate_rays(fma_norm=True) at img_wh with near 2.0 and far 6.0, column 8 = t.  all_rgbs and all_imgs are allocated once; every
    frame's rows and its all_imgs slice are stored in place."""
    from .ray_utils import generate_rays
    perturbation = _check_perturbation(perturbation)
    images = images if isinstance(images, (list, tuple)) else list(images)
    w, h = (int(v) for v in img_wh)
    n, hw = len(images), w * h
    device = torch.device("cuda", torch.cuda.current_device())
    K = intrinsics(camera_angle_x, w, h)
    all_rays = torch.empty(n * hw, 9, dtype=torch.float32, device=device)
    all_rgbs = torch.empty(n * hw, 3, dtype=torch.float32, device=device)
    all_imgs = torch.empty(n, 3, h, w, dtype=torch.float32, device=device)
    for t, im in enumerate(images):
        img = _device_frame(im, device)
        params = perturbation_params(perturbation, t) if t != 0 else None
        _prepare(img, (w, h), params, out="rows", dst=all_rgbs[t * hw:(t + 1) * hw])
        _prepare(img, (w, h), params, out="chw", signed=True, dst=all_imgs[t])
        all_rays[t * hw:(t + 1) * hw, :8] = generate_rays(h, w, K, c2ws[t], NEAR, FAR, device=device, fma_norm=True)
        all_rays[t * hw:(t + 1) * hw, 8] = float(t)
    return all_rays, all_rgbs, all_imgs


def make_eval_sample(img_u8, c2w, camera_angle_x, img_wh, idx, split, perturbation=()):
    """The sample dict of BlenderDataset.__getitem__ for a split other than 'train' (:164-204), built on the device from a decoded frame:
    'rays' [h*w, 8], 'ts' int64 [h*w], 'rgbs' [h*w, 3] (blended on white), 'c2w' (as given), 'valid_mask' bool [h*w] (alpha > 0 of the resized
    frame), 'rgb_idx' = arange(h*w).  split == 'test_train' and idx != 0: the frame is perturbed with seed idx and ts = idx, else ts = 0.
    split == 'test_train' with a non-empty perturbation adds 'original_rgbs' / 'original_valid_mask' of the unperturbed frame."""
    from .ray_utils import generate_rays
    perturbation = _check_perturbation(perturbation)
    img = _device_frame(img_u8)
    w, h = (int(v) for v in img_wh)
    n = w * h
    t, params = 0, None
    if split == 'test_train' and idx != 0:
        t = int(idx)
        params = perturbation_params(perturbation, t)
    rgbs, valid = _prepare(img, (w, h), params, out="rows", valid_mask=True)
    sample = {
        'rays': generate_rays(h, w, intrinsics(camera_angle_x, w, h), c2w, NEAR, FAR, device=img.device, fma_norm=True),
        'ts': torch.full((n,), t, dtype=torch.int64, device=img.device),
        'rgbs': rgbs,
        'c2w': c2w,
        'valid_mask': valid,
        'rgb_idx': torch.arange(n, dtype=torch.int64, device=img.device),
    }
    if split == 'test_train' and perturbation:
        sample['original_rgbs'], sample['original_valid_mask'] = _prepare(img, (w, h), None, out="rows", valid_mask=True)
    return sample


class BlenderGridSampleBatcher:
    """BlenderDataset.__getitem__ (train, :139-163) with the flat buffers resident in HBM and the batch cut out by one HIP gather
    (crnerf_grid_sample_batch_round_f32).  Mirrored: the lattice of :57-58 -- torch.linspace(0, 1 - 1/img_wh[0], side) on BOTH axes --, the
    unseeded np.random.randint for the frame, torch's global CPU generator for scale / offsets, the min_scale_cur schedule and
    (h_sb * h).round(), half to even.  all_rays [n*h*w, 9], all_rgbs [n*h*w, 3] on the device; all_imgs [n, 3, h, w] or None."""

    def __init__(self, all_rays, all_rgbs, all_imgs, img_wh, batch_size=1024, scale_anneal=-1, min_scale=0.25):
        self.all_rays, self.all_rgbs, self.all_imgs = all_rays, all_rgbs, all_imgs
        self.img_wh = (int(img_wh[0]), int(img_wh[1]))
        w, h = self.img_wh
        if w * h > 2 ** 24:
            raise ValueError("BlenderGridSampleBatcher: img_wh %s has more than 2^24 pixels -- the reference's float32 pixel index w + h * img_w "
                             "is inexact beyond that" % (self.img_wh,))
        if all_rays.shape[0] % (w * h) != 0 or all_rays.shape[0] == 0:
            raise ValueError("BlenderGridSampleBatcher: all_rays has %d rows, no multiple of %d x %d" % (all_rays.shape[0], w, h))
        self.n_frames = all_rays.shape[0] // (w * h)
        self.batch_size, self.scale_anneal, self.min_scale = batch_size, scale_anneal, min_scale
        self.iterations = all_rays.shape[0] // batch_size               # :133
        self.side = int(sqrt(batch_size))
        self._lin = torch.linspace(0, 1 - 1 / self.img_wh[0], self.side).to(all_rays.device)

    def __len__(self):
        return self.iterations

    def draw(self, idx, current_epoch=0):
        """The host-side random choices of __getitem__ (:141-148), in the reference's order on the reference's generators."""
        sample_ts = int(np.random.randint(0, self.n_frames))
        if self.scale_anneal > 0:
            min_scale_cur = min(max(self.min_scale, 1. * exp(-(current_epoch * self.iterations + idx) * self.scale_anneal)), 0.9)
        else:
            min_scale_cur = self.min_scale
        scale = torch.Tensor(1).uniform_(min_scale_cur, 1.)
        h_offset = torch.Tensor(1).uniform_(0., (1. - scale.item()) * (1. - 1. / self.img_wh[1]))
        w_offset = torch.Tensor(1).uniform_(0., (1. - scale.item()) * (1. - 1. / self.img_wh[0]))
        return sample_ts, min_scale_cur, float(scale), float(h_offset), float(w_offset)

    def __getitem__(self, idx, current_epoch=0):
        from .. import ops
        sample_ts, min_scale_cur, scale, h_offset, w_offset = self.draw(idx, current_epoch)
        w, h = self.img_wh
        s = ops.grid_sample_batch(self.all_rays, self.all_rgbs, w * h * sample_ts, w, h, self.side, self._lin, self._lin, scale, h_offset,
                                  w_offset, rounding="round")
        s.update({'whole_img': self.all_imgs[sample_ts] if self.all_imgs is not None else None, 'min_scale_cur': min_scale_cur})
        return s

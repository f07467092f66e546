"""Image preparation of the reference's datasets, on the device: PIL.Image.resize(..., Image.LANCZOS) + ToTensor (+ Normalize(0.5, 0.5))
as datasets/phototourism_mask_grid_sample.py:183-199 (training buffers), :288-320 (eval sample) and eval.py:140-151 (style photo) apply
them, bit for bit (csrc/imageprep.hip; the arithmetic is stated in include/crnerf.h and DESIGN 3.6 N7), and the builders on top: a decoded
photo (uint8 HWC) plus its COLMAP camera is all the host supplies.  Reading image files and COLMAP binaries stays outside.

lanczos_coeffs is host-only (float64, numpy): this module imports without the HIP library."""
import math

import numpy as np
import torch

PRECISION_BITS = 22      # Pillow's fixed point of the 8-bit resize


def _lanczos(x):
    if not -3.0 <= x < 3.0:
        return 0.0
    if x == 0.0:
        return 1.0
    a, b = math.pi * x, math.pi * (x / 3.0)
    return (math.sin(a) / a) * (math.sin(b) / b)


def lanczos_coeffs(in_size, out_size):
    """Pillow's coefficient table of one axis, in_size -> out_size, the box being the whole image: (k int32 [out_size, ksize], bounds int32
    [out_size, 2] = (xmin, xmax)).  float64 inside, libm's sin like Pillow's C; asserts that an int32 accumulator holds every output."""
    in_size, out_size = int(in_size), int(out_size)
    if in_size < 1 or out_size < 1:
        raise ValueError("lanczos_coeffs: sizes must be positive, got %d -> %d" % (in_size, out_size))
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support = 3.0 * fs
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / fs
    k = np.zeros((out_size, ksize), dtype=np.int32)
    bounds = np.zeros((out_size, 2), dtype=np.int32)
    one = float(1 << PRECISION_BITS)
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        w = [_lanczos((x + xmin - center + 0.5) * ss) for x in range(xmax)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        k[xx, :xmax] = [int(-0.5 + v * one) if v < 0 else int(0.5 + v * one) for v in w]
        bounds[xx] = (xmin, xmax)
    assert int(np.abs(k.astype(np.int64)).sum(axis=1).max()) * 255 + (1 << (PRECISION_BITS - 1)) < 2 ** 31, \
        "lanczos_coeffs: %d -> %d overflows the int32 accumulator" % (in_size, out_size)
    return k, bounds


def _device_image(img_u8, device=None):
    """The photo as a contiguous uint8 [H, W, 3] device tensor (a host tensor / array is uploaded as it is: one copy of the decoded bytes)."""
    t = torch.as_tensor(img_u8)
    if not t.is_cuda:
        t = t.to(device if device is not None else torch.device("cuda", torch.cuda.current_device()))
    return t.contiguous()


def resize_lanczos(img_u8, size_wh):
    """uint8 [h, w, 3] == PIL.Image.fromarray(img).resize((w, h), Image.LANCZOS)."""
    from .. import ops
    return ops.lanczos_resize(_device_image(img_u8), size_wh, out="u8")


def style_image(img_u8, downscale=8, signed=False):
    """The style / appearance photo at 1/downscale: [1, 3, H//downscale, W//downscale] float32.  signed=True: in [-1, 1], eval.py:142-150
    (resize, ToTensor, Normalize) -- what enc_a sees there; signed=False: in [0, 1], the `style_img` of video.render_video / pipeline.render_frame."""
    from .. import ops
    img = _device_image(img_u8)
    H, W = int(img.shape[0]), int(img.shape[1])
    return ops.lanczos_resize(img, (W // int(downscale), H // int(downscale)), out="chw", signed=signed)[None]


def make_eval_sample(img_u8, K, c2w, near, far, image_id, img_downscale, appearance_downscale=8):
    """The sample dict of PhototourismDataset.__getitem__ for split 'val' / 'test_train' / 'test_test' (:277-320), built on the device from a
    decoded photo: 'c2w' (as given), 'rgbs' [h*w, 3] (the photo at 1/img_downscale, ToTensor, pixel-major), 'rays' [h*w, 8] (generate_rays),
    'ts' int64 [h*w] = image_id, 'img_wh' LongTensor (w, h) on the host, 'rgb_idx' = arange(h*w), 'whole_img' [3, H//a, W//a] in [-1, 1].
    K: the intrinsics already scaled by img_downscale (:96-101).  img_downscale == 1: no resize runs, 'rgbs' is ToTensor of the photo.
    'uv_sample' is not built: nothing in this package reads it (the eval path takes every pixel in order)."""
    from .. import ops
    from .ray_utils import generate_rays
    img = _device_image(img_u8)
    H, W = int(img.shape[0]), int(img.shape[1])
    d, a = int(img_downscale), int(appearance_downscale)
    w, h = (W // d, H // d) if d > 1 else (W, H)
    n = h * w
    return {
        'c2w': c2w,
        'rgbs': ops.lanczos_resize(img, (w, h), out="rows"),
        'rays': generate_rays(h, w, K, c2w, near, far, device=img.device),
        'ts': torch.full((n,), int(image_id), dtype=torch.int64, device=img.device),
        'img_wh': torch.LongTensor([w, h]),
        'rgb_idx': torch.arange(n, dtype=torch.int64, device=img.device),
        'whole_img': ops.lanczos_resize(img, (W // a, H // a), out="chw", signed=True),
    }


def build_train_buffers(images, Ks, c2ws, nears, fars, ids, img_downscale, appearance_downscale=8):
    """The training buffers of PhototourismDataset(split='train') (:180-212) on the device: (all_rays [N, 9], all_rgbs [N, 3], all_imgs_wh
    [n, 2] (float32, host, (w, h) per photo), all_imgs: list of [3, H//a, W//a] in [-1, 1]), ready for
    GridSampleBatcher(all_rays, all_rgbs, all_imgs_wh, all_imgs=all_imgs).
    images: an iterable of decoded photos, uint8 [H, W, 3], on the host or the device; they go through the device one at a time (peak device
    memory: one photo plus the buffers; an iterator is first collected on the host, its sizes being needed to allocate the buffers).  Ks[i]: intrinsics scaled by img_downscale; c2ws[i] [3, 4]; nears / fars / ids: per photo.  The appearance image is
    (W // a, H // a) of the ORIGINAL photo (:194).  all_rgbs is allocated once; every photo's resize stores its rows in place."""
    from .. import ops
    from .ray_utils import generate_rays
    images = images if isinstance(images, (list, tuple)) else list(images)
    d, a = int(img_downscale), int(appearance_downscale)
    sizes = []
    for im in images:
        H, W = int(im.shape[0]), int(im.shape[1])
        sizes.append((W // d, H // d) if d > 1 else (W, H))
    device = torch.device("cuda", torch.cuda.current_device())
    N = sum(w * h for w, h in sizes)
    all_rays = torch.empty(N, 9, dtype=torch.float32, device=device)
    all_rgbs = torch.empty(N, 3, dtype=torch.float32, device=device)
    all_imgs, row = [], 0
    for i, im in enumerate(images):
        img = _device_image(im, device)
        H, W = int(img.shape[0]), int(img.shape[1])
        w, h = sizes[i]
        n = w * h
        ops.lanczos_resize(img, (w, h), out="rows", dst=all_rgbs[row:row + n])
        all_imgs.append(ops.lanczos_resize(img, (W // a, H // a), out="chw", signed=True))
        all_rays[row:row + n, :8] = generate_rays(h, w, Ks[i], c2ws[i], float(nears[i]), float(fars[i]), device=device)
        all_rays[row:row + n, 8] = float(ids[i])
        row += n
    all_imgs_wh = torch.tensor([[float(w), float(h)] for w, h in sizes], dtype=torch.float32).reshape(-1, 2)
    return all_rays, all_rgbs, all_imgs_wh, all_imgs

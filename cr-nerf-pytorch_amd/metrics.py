"""Mirror of the reference's metrics.py (mse / psnr / ssim, same names and signatures) on crnerf_image_metrics_f32
(csrc/metrics.hip): one launch reads the image pair once and gives the sum of squared differences, the sum of the
SSIM map and, on request, the map.  kornia is not needed: its ssim(img1, img2, 3) is restated in include/crnerf.h.

    mse, psnr, ssim          metrics.py:4-20
    image_metrics(...)       all three from ONE launch, optionally on the right half eval_metric.py:87-93 scores and with the
                             prediction taken through the uint8 round trip of the reference's PNG files (eval.py:296-297)

GPU tensors only: like every op of the package there is no CPU fallback.
"""
import torch

from . import ops


def _as_chw(t):
    """mse / psnr take what the reference hands them: (1,C,H,W), (C,H,W), (H,W,3) slices, [R,3].  The mean over all elements does
    not care which axis is called what, so the tensor is read in place as a <= 3-D grid (missing leading axes have size 1)."""
    if torch.is_tensor(t):
        if t.dim() == 4 and t.shape[0] == 1:
            t = t[0]
        while t.dim() < 3:
            t = t[None]
    return t


def _sums(image_pred, image_gt):
    return ops.image_metrics(_as_chw(image_pred), _as_chw(image_gt))


def mse(image_pred, image_gt, valid_mask=None, reduction='mean'):
    if valid_mask is not None or reduction != 'mean':
        raise NotImplementedError("crnerf_amd: mse / psnr implement valid_mask=None, reduction='mean' (what the reference's callers use)")
    sse, _, n, _ = _sums(image_pred, image_gt)
    return (sse / n).to(torch.float32)


def psnr(image_pred, image_gt, valid_mask=None, reduction='mean'):
    if valid_mask is not None or reduction != 'mean':
        raise NotImplementedError("crnerf_amd: mse / psnr implement valid_mask=None, reduction='mean' (what the reference's callers use)")
    sse, _, n, _ = _sums(image_pred, image_gt)
    return (-10.0 * torch.log10(sse / n)).to(torch.float32)


def ssim(image_pred, image_gt, reduction='mean'):
    """
    image_pred and image_gt: (1, 3, H, W)
    Returns the SSIM map (1, 3, H, W); `reduction` is ignored, as in the reference.
    """
    if not torch.is_tensor(image_pred) or image_pred.dim() != 4:
        raise ValueError("crnerf_amd: ssim takes (B,C,H,W) images")
    if image_pred.shape != image_gt.shape:
        raise ValueError("crnerf_amd: image_pred %s and image_gt %s differ in shape" % (tuple(image_pred.shape), tuple(image_gt.shape)))
    maps = [ops.image_metrics(image_pred[b], image_gt[b], want_map=True)[3] for b in range(image_pred.shape[0])]
    return maps[0][None] if len(maps) == 1 else torch.stack(maps, 0)


def image_metrics(image_pred, image_gt, half=None, quantize_pred=False):
    """{'mse', 'psnr', 'ssim'} (0-dim float32 device tensors; ssim = mean of the map) of a (1,C,H,W) / (C,H,W) image pair from one
    launch.  half='right': the region x >= W // 2 that eval_metric.py:90-93 scores on Phototourism test images (the other half
    gave the appearance); the SSIM border is reflected inside that half, as the reference crops before it filters.
    quantize_pred=True: the prediction as the reference's PNG holds it (clip to [0,1], * 255, truncate to uint8, / 255)."""
    if half not in (None, 'right'):
        raise ValueError("crnerf_amd: half must be None or 'right'")
    roi = None
    if half == 'right':
        H, W = (int(v) for v in image_pred.shape[-2:])
        roi = (W // 2, 0, W - W // 2, H)
    sse, ssim_sum, n, _ = ops.image_metrics(image_pred, image_gt, roi=roi, quantize_pred=quantize_pred)
    m = sse / n
    return {'mse': m.to(torch.float32), 'psnr': (-10.0 * torch.log10(m)).to(torch.float32), 'ssim': (ssim_sum / n).to(torch.float32)}


__all__ = ["mse", "psnr", "ssim", "image_metrics"]

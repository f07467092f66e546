"""Mirror of the reference's metrics.py (mse / psnr / ssim, same names and signatures) on crnerf_image_metrics_f32
(csrc/metrics.hip): one launch reads the image pair once and gives the sum of squared differences, the sum of the
SSIM map and, on request, the map.  kornia is not needed: its ssim(img1, img2, 3) is restated in include/crnerf.h.

    mse, psnr, ssim          metrics.py:4-20
    image_metrics(...)       all three from ONE launch, optionally on the right half eval_metric.py:87-93 scores and with the
                             prediction taken through the uint8 round trip of the reference's PNG files (eval.py:296-297)
    lpips(...)               eval_metric.py:92, lpips.LPIPS(net='alex'), on crnerf_lpips_f32 (csrc/lpips.hip); the network's weights are
                             not shipped: load_lpips_weights reads them from the files of an lpips / torchvision install

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


LPIPS_SHIFT = (-.030, -.088, -.188)       # lpips.ScalingLayer's buffers
LPIPS_SCALE = (.458, .448, .450)
_ALEX_LAYERS = ((0, 64, 3, 11), (3, 192, 64, 5), (6, 384, 192, 3), (8, 256, 384, 3), (10, 256, 256, 3))   # features index, cout, cin, k


class LPIPSWeights:
    """The 17 float32 device tensors crnerf_lpips_f32 reads: conv_w[5] ([cout,cin,k,k], the modules' own layout), conv_b[5], lin[5]
    ([C_l]), shift[3], scale[3].  Built by load_lpips_weights."""

    def __init__(self, conv_w, conv_b, lin, shift, scale):
        self.conv_w, self.conv_b, self.lin, self.shift, self.scale = list(conv_w), list(conv_b), list(lin), shift, scale

    def tensors(self):
        return self.conv_w + self.conv_b + self.lin + [self.shift, self.scale]


def _lpips_take(state, names, shape, what):
    for name in names:
        if name in state:
            t = state[name]
            if not torch.is_tensor(t) or tuple(t.shape) != tuple(shape):
                raise ValueError("crnerf_amd: LPIPS weight %r has shape %s, expected %s"
                                 % (name, tuple(t.shape) if torch.is_tensor(t) else type(t).__name__, tuple(shape)))
            return t
    raise KeyError("crnerf_amd: LPIPS weights: %s is missing (looked for %s)" % (what, " / ".join(repr(n) for n in names)))


def load_lpips_weights(src, lin=None, device="cuda"):
    """LPIPSWeights from `src` (and `lin`): each a state dict or a path read with torch.load(..., weights_only=True).  Two key
    conventions are accepted:
      1. the state dict of lpips.LPIPS(net='alex'): net.slice1.0.*, net.slice2.3.*, net.slice3.6.*, net.slice4.8.*, net.slice5.10.*
         (weight / bias), lin{0..4}.model.1.weight of shape [1,C,1,1] (the lins.{i}.model.1.weight aliases are tolerated) and
         scaling_layer.shift / scaling_layer.scale;
      2. a torchvision AlexNet state dict (features.{0,3,6,8,10}.weight / .bias) plus lin=, the lpips package's weights/v0.1/alex.pth,
         which holds lin{i}.model.1.weight only.
    shift and scale default to the package's constants (LPIPS_SHIFT, LPIPS_SCALE) when the dict has none.  A missing key raises
    KeyError, a wrong shape ValueError, both naming the key.
    These key names are written from knowledge of lpips 0.1.x and torchvision; neither package was available where this was written,
    so they have NOT been checked against the real files."""
    def as_dict(s, what):
        if isinstance(s, (str, bytes)) or hasattr(s, "__fspath__"):
            s = torch.load(s, map_location="cpu", weights_only=True)
        if not hasattr(s, "keys"):
            raise TypeError("crnerf_amd: %s must be a state dict or a path to one" % what)
        return s
    state = as_dict(src, "src")
    lin_state = as_dict(lin, "lin") if lin is not None else state
    conv_w, conv_b, lins = [], [], []
    for i, (idx, cout, cin, k) in enumerate(_ALEX_LAYERS):
        names = ["net.slice%d.%d." % (i + 1, idx), "features.%d." % idx]
        conv_w.append(_lpips_take(state, [n + "weight" for n in names], (cout, cin, k, k), "conv%d's weight" % (i + 1)))
        conv_b.append(_lpips_take(state, [n + "bias" for n in names], (cout,), "conv%d's bias" % (i + 1)))
        lins.append(_lpips_take(lin_state, ["lin%d.model.1.weight" % i, "lins.%d.model.1.weight" % i], (1, cout, 1, 1), "lin%d" % i).reshape(cout))
    consts = []
    for name, default in (("shift", LPIPS_SHIFT), ("scale", LPIPS_SCALE)):
        key = "scaling_layer." + name
        if key in state:
            t = state[key]
            if not torch.is_tensor(t) or t.numel() != 3:
                raise ValueError("crnerf_amd: LPIPS weight %r has shape %s, expected 3 elements" % (key, tuple(t.shape) if torch.is_tensor(t) else type(t).__name__))
            consts.append(t.reshape(3))
        else:
            consts.append(torch.tensor(default, dtype=torch.float32))
    put = lambda t: t.detach().to(device=device, dtype=torch.float32).contiguous().clone()  # noqa: E731  own, aligned storage
    return LPIPSWeights([put(t) for t in conv_w], [put(t) for t in conv_b], [put(t) for t in lins], put(consts[0]), put(consts[1]))


def lpips(image_pred, image_gt, weights, half=None, quantize_pred=False, normalize=True):
    """LPIPS (AlexNet) of a (1,3,H,W) / (3,H,W) image pair as a 0-dim float32 device tensor (ops.lpips's total).  half='right': the
    region x >= W // 2 of image_metrics, cropped BEFORE the network sees it as eval_metric.py:90-92 does (the zero padding of conv1
    sits at the crop's border; nothing is copied).  quantize_pred: the prediction as the reference's PNG holds it.  normalize: the
    images are in [0,1] and are mapped to [-1,1] first (eval_metric.py:92's * 2 - 1); False takes them as already in [-1,1]."""
    if half not in (None, 'right'):
        raise ValueError("crnerf_amd: half must be None or 'right'")
    roi = None
    if half == 'right':
        H, W = (int(v) for v in image_pred.shape[-2:])
        roi = (W // 2, 0, W - W // 2, H)
    total, _, _ = ops.lpips(image_pred, image_gt, weights, roi=roi, quantize_pred=quantize_pred, normalize=normalize)
    return total.to(torch.float32)


__all__ = ["mse", "psnr", "ssim", "image_metrics", "lpips", "LPIPSWeights", "load_lpips_weights"]

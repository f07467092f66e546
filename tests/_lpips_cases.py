"""The float64 restatement of LPIPS (AlexNet backbone, version 0.1; include/crnerf.h carries the definition) that
tests/test_lpips_host.py pins analytically and tests/test_gpu_lpips.py holds csrc/lpips.hip to, plus the weight sets both use.
torch.nn.functional.conv2d / max_pool2d on the CPU; neither the lpips package nor torchvision is installed anywhere this suite runs,
so nothing here has been compared with them."""
import torch
import torch.nn.functional as F

SHIFT = (-.030, -.088, -.188)
SCALE = (.458, .448, .450)
LAYERS = ((64, 3, 11, 4, 2), (192, 64, 5, 1, 2), (384, 192, 3, 1, 1), (256, 384, 3, 1, 1), (256, 256, 3, 1, 1))   # cout, cin, k, stride, pad
FEATURE_INDEX = (0, 3, 6, 8, 10)                       # torchvision AlexNet .features indices of the five convolutions
CHANNELS = tuple(l[0] for l in LAYERS)
EPS = 1e-10


def map_sizes(h, w):
    """[(h_l, w_l)] of F1..F5, written out by hand: conv1 (n - 7) // 4 + 1, each pool (m - 3) // 2 + 1."""
    s1 = ((h - 7) // 4 + 1, (w - 7) // 4 + 1)
    s2 = ((s1[0] - 3) // 2 + 1, (s1[1] - 3) // 2 + 1)
    s3 = ((s2[0] - 3) // 2 + 1, (s2[1] - 3) // 2 + 1)
    return [s1, s2, s3, s3, s3]


def scaling(x, w, dtype=torch.float64, normalize=True):
    """(N,3,H,W) images -> the network's input: optional * 2 - 1, then (x - shift) / scale in `dtype`."""
    x = x.to(dtype)
    if normalize:
        x = x * 2 - 1
    return (x - w["shift"].to(dtype).view(1, 3, 1, 1)) / w["scale"].to(dtype).view(1, 3, 1, 1)


def features(s, w, dtype=torch.float64):
    """F1..F5 ((N,C_l,h_l,w_l), in `dtype`) of the scaled input s."""
    out, x = [], s.to(dtype)
    for l, (cout, cin, k, stride, pad) in enumerate(LAYERS):
        if l in (1, 2):
            x = F.max_pool2d(x, 3, 2)
        x = F.relu(F.conv2d(x, w["conv_w"][l].to(dtype), w["conv_b"][l].to(dtype), stride=stride, padding=pad))
        out.append(x)
    return out


def head(f0, f1, lin, dtype=torch.float64):
    """[5] tensor of d_l from the two images' maps (lists of (1,C,h,w) or (C,h,w)) and the lin weights ([C] each)."""
    d = []
    for a, b, wl in zip(f0, f1, lin):
        a, b = a.to(dtype).reshape(wl.numel(), -1), b.to(dtype).reshape(wl.numel(), -1)
        na = a / (a.pow(2).sum(0, keepdim=True).sqrt() + EPS)
        nb = b / (b.pow(2).sum(0, keepdim=True).sqrt() + EPS)
        d.append((wl.to(dtype)[:, None] * (na - nb) ** 2).sum(0).mean())
    return torch.stack(d)


def lpips(x0, x1, w, dtype=torch.float64, normalize=True):
    """(total, d[5], F(x0), F(x1)) of two (1,3,H,W) images."""
    f = features(scaling(torch.cat([x0, x1], 0), w, dtype, normalize), w, dtype)
    f0, f1 = [t[0:1] for t in f], [t[1:2] for t in f]
    d = head(f0, f1, w["lin"], dtype)
    return d.sum(), d, f0, f1


def rel_l2(a, ref):
    return float((a.double() - ref.double()).norm() / ref.double().norm())


# ------------------------------------------------------------------ weight sets (CPU float32 dicts)
def exact_weights(seed=5, lin_seed=None):
    """Exactly summable: every weight row has exactly 8 non-zero entries of +-1 at random positions, biases in {-1, 0, 1}, shift 0,
    scale 1.  With image values in {-1, -.5, 0, .5, 1} (normalize=False) every partial sum, in any order, is a multiple of 1/2 below
    2^17, so fp32 in any summation order gives the float64 maps exactly.  lin: ones, or non-negative uniform values (lin_seed)."""
    g = torch.Generator().manual_seed(seed)
    w = {"conv_w": [], "conv_b": [], "lin": [], "shift": torch.zeros(3), "scale": torch.ones(3)}
    for cout, cin, k, _, _ in LAYERS:
        K = cin * k * k
        rows = torch.zeros(cout, K)
        for o in range(cout):
            pos = torch.randperm(K, generator=g)[:8]
            rows[o, pos] = (torch.randint(0, 2, (8,), generator=g) * 2 - 1).float()
        w["conv_w"].append(rows.reshape(cout, cin, k, k))
        w["conv_b"].append(torch.randint(-1, 2, (cout,), generator=g).float())
    gl = torch.Generator().manual_seed(lin_seed) if lin_seed is not None else None
    w["lin"] = [torch.rand(c, generator=gl) if gl is not None else torch.ones(c) for c in CHANNELS]
    return w


def exact_image(H, W, seed):
    """(1,3,H,W) with values in {-1, -.5, 0, .5, 1}"""
    g = torch.Generator().manual_seed(seed)
    return (torch.randint(0, 5, (1, 3, H, W), generator=g).float() - 2) / 2


def gaussian_weights(seed=11):
    """Gaussian weights of std 1.4 / sqrt(K) (activations keep their scale through the five layers), biases of std 0.1, non-negative
    lin, the package's shift / scale."""
    g = torch.Generator().manual_seed(seed)
    w = {"conv_w": [], "conv_b": [], "lin": [], "shift": torch.tensor(SHIFT), "scale": torch.tensor(SCALE)}
    for cout, cin, k, _, _ in LAYERS:
        w["conv_w"].append(torch.randn(cout, cin, k, k, generator=g) * (1.4 / (cin * k * k) ** 0.5))
        w["conv_b"].append(torch.randn(cout, generator=g) * 0.1)
        w["lin"].append(torch.rand(cout, generator=g))
    return w


def dead_weights():
    """All weights 0, all biases -1: every feature of every layer is relu(-1) = 0."""
    w = {"conv_w": [torch.zeros(cout, cin, k, k) for cout, cin, k, _, _ in LAYERS], "conv_b": [-torch.ones(c) for c in CHANNELS],
         "lin": [torch.ones(c) for c in CHANNELS], "shift": torch.tensor(SHIFT), "scale": torch.tensor(SCALE)}
    return w


def lpips_state_dict(w, scaling_layer=True, lins_alias=False):
    """The weight set under the key names of lpips.LPIPS(net='alex').state_dict() (as written in metrics.load_lpips_weights)."""
    sd = {}
    for l, idx in enumerate(FEATURE_INDEX):
        sd["net.slice%d.%d.weight" % (l + 1, idx)] = w["conv_w"][l]
        sd["net.slice%d.%d.bias" % (l + 1, idx)] = w["conv_b"][l]
        sd[("lins.%d.model.1.weight" if lins_alias else "lin%d.model.1.weight") % l] = w["lin"][l].reshape(1, -1, 1, 1)
    if scaling_layer:
        sd["scaling_layer.shift"] = w["shift"].reshape(1, 3, 1, 1)
        sd["scaling_layer.scale"] = w["scale"].reshape(1, 3, 1, 1)
    return sd


def torchvision_state_dicts(w):
    """(torchvision AlexNet features state dict, the lpips package's weights/v0.1/alex.pth contents)"""
    tv, lin = {}, {}
    for l, idx in enumerate(FEATURE_INDEX):
        tv["features.%d.weight" % idx] = w["conv_w"][l]
        tv["features.%d.bias" % idx] = w["conv_b"][l]
        lin["lin%d.model.1.weight" % l] = w["lin"][l].reshape(1, -1, 1, 1)
    return tv, lin

"""Numpy restatement of the Blender dataset's frame preparation (the arithmetic of DESIGN 3.6 N9, nothing cleverer) and the seeded inputs
of the Blender tests: the occluders and the colour table of add_perturbation, Pillow's RGBA resize = premultiply, the 8-bit LANCZOS passes
of tests/_lanczos_cases.py on four channels, un-premultiply; then the reference's float32 expressions in torch on the CPU.
tests/golden/make_golden_blender.py stores what Pillow and the reference themselves give on these inputs."""
import os

import numpy as np
import torch

import _lanczos_cases as L

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g19_blender.npz")
PATTERNS = ("noise", "edges", "blocks")
# the blocks cases on which Pillow's own output must hold >= 10 % of alpha 0, >= 10 % of alpha 255 and >= 10 % strictly between
SHARES = ("odd_half", "vertical_only", "horizontal_only", "identity", "upscale")


# ---- the arithmetic --------------------------------------------------------------------------------------------------------------

def premultiply(a):
    """Pillow's RGBA -> RGBa: t = c * a + 128, c' = ((t >> 8) + t) >> 8; alpha kept."""
    out = a.copy()
    t = a[..., :3].astype(np.uint32) * a[..., 3:].astype(np.uint32) + 128
    out[..., :3] = ((t >> 8) + t) >> 8
    return out


def unpremultiply(a):
    """Pillow's RGBa -> RGBA: c for alpha 0 or 255, else min(255, (255 * c) // alpha).  Returns (image, colour bytes that hit the min)."""
    out = a.copy()
    al = a[..., 3:].astype(np.int64)
    q = (255 * a[..., :3].astype(np.int64)) // np.maximum(al, 1)
    mid = (al != 0) & (al != 255)
    out[..., :3] = np.where(mid, np.minimum(q, 255), a[..., :3])
    return out, int((mid & (q > 255)).sum())


def resize_premultiplied(a, size_wh):
    """The premultiplied image after the passes: what the un-premultiply sees."""
    w, h = size_wh
    H, W = a.shape[:2]
    a = premultiply(a)
    if w != W:
        a = L.one_pass(a.transpose(1, 0, 2), *L.coeffs(W, w)).transpose(1, 0, 2)
    if h != H:
        a = L.one_pass(a, *L.coeffs(H, h))
    return np.ascontiguousarray(a)


def resize(a, size_wh):
    """a: uint8 [H, W, 4] -> uint8 [h, w, 4] == Image.fromarray(a).resize((w, h), Image.LANCZOS); an unchanged size is a copy."""
    if tuple(size_wh) == (a.shape[1], a.shape[0]):
        return a.copy()
    return unpremultiply(resize_premultiplied(a, size_wh))[0]


def clip_count(a, size_wh):
    if tuple(size_wh) == (a.shape[1], a.shape[0]):
        return 0
    return unpremultiply(resize_premultiplied(a, size_wh))[1]


def paint(a, rects, colors):
    """ImageDraw.rectangle(((x0, y0), (x1, y1)), fill=rgb) on RGBA, in order: inclusive bounds, clipped, alpha 255."""
    out = a.copy()
    H, W = a.shape[:2]
    for (x0, y0, x1, y1), c in zip(np.asarray(rects).reshape(-1, 4), np.asarray(colors).reshape(-1, 3)):
        xa, xb, ya, yb = max(int(x0), 0), min(int(x1), W - 1), max(int(y0), 0), min(int(y1), H - 1)
        if xa <= xb and ya <= yb:
            out[ya:yb + 1, xa:xb + 1] = (int(c[0]), int(c[1]), int(c[2]), 255)
    return out


def apply_lut(a, lut):
    out = a.copy()
    if lut is not None:
        for c in range(3):
            out[..., c] = np.asarray(lut)[c][a[..., c]]
    return out


def perturb(a, rects, colors, lut):
    return apply_lut(paint(a, rects, colors), lut)


def color_table(s, b):
    """(255 * np.clip(s * (v / 255.0) + b, 0, 1)).astype(np.uint8) for v = 0 ... 255, per channel: [3, 256]."""
    v = np.arange(256) / 255.0
    return np.stack([(255 * np.clip(s[c] * v + b[c], 0, 1)).astype(np.uint8) for c in range(3)])


def tensors(u8):
    """The reference's float32 expressions on the CPU (:107-110, :175-178): {'rows' [h*w, 3], 'chw' [3, h, w], 'signed' [3, h, w],
    'valid' bool [h*w]} of a uint8 [h, w, 4] frame."""
    img = torch.from_numpy(np.ascontiguousarray(u8)).permute(2, 0, 1).contiguous().to(torch.float32).div(255)      # ToTensor
    valid = (img[-1] > 0).flatten()
    img = img[:3, :, :] * img[-1:, :, :] + (1 - img[-1:, :, :])
    half = torch.tensor([0.5, 0.5, 0.5])[:, None, None]
    return {"rows": img.reshape(3, -1).permute(1, 0).contiguous(), "chw": img, "signed": img.clone().sub_(half).div_(half), "valid": valid}


# ---- inputs ----------------------------------------------------------------------------------------------------------------------

def make_input(pattern, seed, H, W):
    g = np.random.default_rng(seed)
    a = g.integers(0, 256, (H, W, 4), dtype=np.uint8)
    if pattern == "edges":
        a[..., 3] = np.array([0, 255, 1, 254, 128], dtype=np.uint8)[g.integers(0, 5, (H, W))]
    elif pattern == "blocks":
        blk = np.array([0, 255, 3], dtype=np.uint8)[g.integers(0, 3, ((H + 8) // 9, (W + 8) // 9))]
        a[..., 3] = np.repeat(np.repeat(blk, 9, axis=0), 9, axis=1)[:H, :W]
    return a


def table_cases():
    """[(key, pattern, seed, H, W, w, h)]: every shape of _lanczos_cases.SHAPES on the three alpha patterns."""
    cases = []
    for i, (name, H, W, w, h, _) in enumerate(L.SHAPES):
        for j, pat in enumerate(PATTERNS):
            cases.append(("%s_%s" % (name, pat), pat, 1000 + 10 * i + j, H, W, w, h))
    return cases


def case_input(case):
    return make_input(case[1], case[2], case[3], case[4])


FRAME = 640                      # side of the synthetic frames of the perturbation / dataset fixtures
IMG_WH = (40, 40)
PERTURB_SEEDS = (1, 2, 7)
PERTURB_SETS = (("occ",), ("color",), ("occ", "color"))
CAMERA_ANGLE_X = 0.6911112070083618
N_FRAMES = 3


def frame(seed, side=FRAME):
    """A synthetic Blender-like frame: an object (alpha 255) on nothing (alpha 0, colour 0) with a soft rim, noise-textured colour."""
    g = np.random.default_rng(5000 + seed)
    y, x = np.mgrid[0:side, 0:side].astype(np.float64)
    cx, cy, r = side * (0.45 + 0.03 * (seed % 3)), side * 0.5, side * (0.3 + 0.02 * (seed % 3))
    d = np.sqrt((x - cx) ** 2 + (y - cy) ** 2)
    alpha = np.clip((r - d) / 6.0 + 0.5, 0, 1)
    col = (g.integers(0, 256, (side, side, 3)) // 2 + (np.stack([x, y, x + y], -1) * (127.0 / (2 * side)))).astype(np.uint8)
    a = np.zeros((side, side, 4), dtype=np.uint8)
    a[..., 3] = np.round(alpha * 255)
    a[..., :3] = np.where(a[..., 3:] > 0, col, 0)
    return a


def poses():
    """float32 [N_FRAMES, 3, 4]: cameras on a ring of radius 4 looking at the origin."""
    out = []
    for t in range(N_FRAMES):
        th = 0.7 * t + 0.3
        eye = np.array([4 * np.cos(th), 4 * np.sin(th), 1.0 + 0.5 * t])
        z = eye / np.linalg.norm(eye)
        x = np.cross([0.0, 0.0, 1.0], z)
        x /= np.linalg.norm(x)
        out.append(np.concatenate([np.stack([x, np.cross(z, x), z], 1), eye[:, None]], 1))
    return np.stack(out).astype(np.float32)


def load_golden():
    """The fixture, after checking each regenerated input's byte sum against the recorded one."""
    z = np.load(GOLDEN)
    keys = [str(k) for k in z["keys"]]
    cases = {c[0]: c for c in table_cases()}
    assert sorted(keys) == sorted(cases), "tests/golden/g19_blender.npz and table_cases() disagree: regenerate the fixture"
    for k, s in zip(keys, z["input_sums"]):
        assert int(case_input(cases[k]).sum(dtype=np.int64)) == int(s), "input generator drifted for %s" % k
    for t, s in enumerate(z["frame_sums"]):
        assert int(frame(t).sum(dtype=np.int64)) == int(s), "frame generator drifted for frame %d" % t
    return z

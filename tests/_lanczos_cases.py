"""Numpy restatement of Pillow's 8-bit LANCZOS resize (the arithmetic of DESIGN 3.6 N7, nothing cleverer) and the seeded
inputs of the Lanczos tests.  tests/golden/make_golden_lanczos.py stores what Pillow itself gives on these inputs."""
import math
import os

import numpy as np

PRECISION_BITS = 22
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g17_lanczos.npz")


def lanczos(x):
    def sinc(v):
        return 1.0 if v == 0.0 else math.sin(math.pi * v) / (math.pi * v)
    return sinc(x) * sinc(x / 3.0) if -3.0 <= x < 3.0 else 0.0


def coeffs(in_size, out_size):
    """(k int32 [out, ksize], bounds int32 [out, 2] = (xmin, xmax)) of one axis; the box is the whole image."""
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support = 3.0 * fs
    ksize = int(math.ceil(support)) * 2 + 1
    k = np.zeros((out_size, ksize), dtype=np.int32)
    bounds = np.zeros((out_size, 2), dtype=np.int32)
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        ss = 1.0 / fs
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        w = [lanczos((x + xmin - center + 0.5) * ss) for x in range(xmax)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        for x, v in enumerate(w):
            k[xx, x] = int(-0.5 + v * (1 << PRECISION_BITS)) if v < 0 else int(0.5 + v * (1 << PRECISION_BITS))
        bounds[xx] = (xmin, xmax)
    return k, bounds


def one_pass(a, k, bounds):
    """Resample axis 0 of the uint8 array a [n, ...] -> [out, ...]."""
    out = np.empty((k.shape[0],) + a.shape[1:], dtype=np.uint8)
    wide = a.astype(np.int64)
    for xx in range(k.shape[0]):
        xmin, xmax = (int(v) for v in bounds[xx])
        acc = (1 << (PRECISION_BITS - 1)) + np.tensordot(k[xx, :xmax].astype(np.int64), wide[xmin:xmin + xmax], axes=(0, 0))
        assert np.abs(acc).max() < 2 ** 31                     # the int32 accumulator of the C code and of the kernel
        out[xx] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return out


def resize(a, size_wh):
    """a: uint8 [H, W, 3] -> uint8 [h, w, 3]; horizontal pass first, uint8 in between, a pass that keeps its size is skipped."""
    w, h = size_wh
    H, W = a.shape[:2]
    if w != W:
        a = one_pass(a.transpose(1, 0, 2), *coeffs(W, w)).transpose(1, 0, 2)
    if h != H:
        a = one_pass(a, *coeffs(H, h))
    return np.ascontiguousarray(a)


# ---- inputs ----------------------------------------------------------------------------------------------------------------------

def noise(seed, H, W):
    return np.random.default_rng(seed).integers(0, 256, (H, W, 3), dtype=np.uint8)


def blocks(seed, H, W, side):
    """0 / 255 blocks of side x side pixels, drawn per channel."""
    g = np.random.default_rng(seed).integers(0, 2, ((H + side - 1) // side, (W + side - 1) // side, 3), dtype=np.uint8) * 255
    return np.ascontiguousarray(np.repeat(np.repeat(g, side, axis=0), side, axis=1)[:H, :W])


def ramp(H, W):
    y, x = np.arange(H)[:, None, None], np.arange(W)[None, :, None]
    return ((x * 255 // max(W - 1, 1) + y * 255 // max(H - 1, 1) + np.arange(3)[None, None, :] * 40) % 256).astype(np.uint8)


def white(H, W):
    return np.full((H, W, 3), 255, dtype=np.uint8)


# (name, H, W, w, h, side of the blocky input: at least 3 x the larger downscale): the table of the issue; the tile shapes are appended by
# the GPU test from the exported constants
SHAPES = [
    ("clipped", 8, 8, 1, 1, 24),
    ("wide_kernel", 31, 47, 5, 3, 32),
    ("odd_half", 67, 93, 46, 33, 8),
    ("eighth", 129, 257, 32, 16, 32),
    ("vertical_only", 40, 40, 40, 20, 6),
    ("horizontal_only", 33, 50, 25, 33, 6),
    ("identity", 33, 50, 50, 33, 4),
    ("upscale", 21, 17, 34, 42, 4),
    ("blocky_half", 70, 131, 65, 35, 6),
    ("blocky_eighth", 131, 70, 8, 16, 24),
]
# the blocky cases on which Pillow's own output must saturate on >= 20 % of the bytes and stay strictly inside on >= 20 %
SHARES = ("odd_half_blocks", "eighth_blocks", "blocky_half_blocks", "blocky_eighth_blocks")
PHOTO = (700, 1000)


def block_side(H, W, w, h):
    """Side of the blocky input of a shape outside the table: above 3 x the larger downscale, at least 4."""
    return max(4, int(math.ceil(3 * max(H / h, W / w, 1.0))) + 1)


def make_input(kind, seed, H, W, w, h, side=None):
    if kind == "noise":
        return noise(seed, H, W)
    if kind == "blocks":
        return blocks(seed, H, W, side or block_side(H, W, w, h))
    return ramp(H, W) if kind == "ramp" else white(H, W)


def golden_cases():
    """[(key, kind, seed, H, W, w, h, side)]: what the fixture holds.  Every table shape on noise and blocks, ramp and white on two."""
    cases = []
    for i, (name, H, W, w, h, side) in enumerate(SHAPES):
        cases.append(("%s_noise" % name, "noise", 100 + i, H, W, w, h, 0))
        cases.append(("%s_blocks" % name, "blocks", 200 + i, H, W, w, h, side))
    for name, H, W, w, h, _ in (SHAPES[2], SHAPES[3]):
        cases.append(("%s_ramp" % name, "ramp", 0, H, W, w, h, 0))
        cases.append(("%s_white" % name, "white", 0, H, W, w, h, 0))
    return cases


def case_input(case):
    key, kind, seed, H, W, w, h, side = case
    return make_input(kind, seed, H, W, w, h, side)


def load_golden():
    """{key: PIL's uint8 [h, w, 3]}, after checking each regenerated input's byte sum against the fixture's."""
    z = np.load(GOLDEN)
    keys = [str(k) for k in z["keys"]]
    cases = {c[0]: c for c in golden_cases()}
    assert sorted(keys) == sorted(cases), "tests/golden/g17_lanczos.npz and golden_cases() disagree: regenerate the fixture"
    for k, s in zip(keys, z["input_sums"]):
        assert int(case_input(cases[k]).sum(dtype=np.int64)) == int(s), "input generator drifted for %s" % k
    return {k: z["out_" + k] for k in keys}

"""Call time of crnerf_amd.ops.rgba_prepare on the GPU for an 800 x 800 RGBA frame: -> 400 x 400 and -> 100 x 100 (rows store + valid_mask,
the rgbs layout), each with and without both perturbations (ten occluders + colour table), and the identity conversion at 800 x 800; the
three-channel ops.lanczos_resize at the same sizes on the same build -- the yardstick for a path that moves 4/3 of its bytes --; and, where
Pillow is installed, the same RGBA resizes + the blend through Pillow / torch on this host.  Device events around every call, median / min /
max of the steady state after a warm-up.  No roofline is claimed.

    python tools/blender_prep_timing.py [--calls 50] [--warmup 10] [--out FILE]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from crnerf_amd import ops  # noqa: E402
from crnerf_amd.datasets import blender  # noqa: E402

SIDE = 800


def timed(fn, calls, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(calls)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    t = sorted(a.elapsed_time(b) * 1e3 for a, b in ev)
    return statistics.median(t), t[0], t[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("blender_prep_timing: needs a GPU")
    dev = "cuda:0"
    rng = np.random.default_rng(0)
    host = rng.integers(0, 256, (SIDE, SIDE, 4), dtype=np.uint8)
    host[..., 3] = np.array([0, 255, 128], dtype=np.uint8)[rng.integers(0, 3, (SIDE // 8, SIDE // 8))].repeat(8, 0).repeat(8, 1)
    src4 = torch.from_numpy(host).to(dev)
    src3 = torch.from_numpy(np.ascontiguousarray(host[..., :3])).to(dev)
    rects, colors, lut = blender.perturbation_params(["occ", "color"], 3)
    lut_dev = torch.from_numpy(lut).to(dev)
    lines = ["blender_prep_timing: %s, %d calls after %d warm-up calls, device events per call, microseconds (median / min / max)"
             % (torch.cuda.get_device_name(0), args.calls, args.warmup)]
    medians = {}
    for side in (400, 100):
        for name, kw in (("plain", {}), ("occ + color", dict(rects=rects, colors=colors, lut=lut_dev))):
            med, lo, hi = timed(lambda: ops.rgba_prepare(src4, (side, side), out="rows", valid_mask=True, **kw), args.calls, args.warmup)
            lines.append("rgba_prepare   800x800x4 -> %3dx%-3d rows + valid_mask, %-11s (2 launches)   %8.1f / %8.1f / %8.1f" % (side, side, name, med, lo, hi))
            medians[("rgba", side, name)] = med
        med, lo, hi = timed(lambda: ops.lanczos_resize(src3, (side, side), out="rows"), args.calls, args.warmup)
        lines.append("lanczos_resize 800x800x3 -> %3dx%-3d rows                             (2 launches)   %8.1f / %8.1f / %8.1f" % (side, side, med, lo, hi))
        medians[("rgb", side)] = med
    med, lo, hi = timed(lambda: ops.rgba_prepare(src4, (SIDE, SIDE), out="rows", valid_mask=True), args.calls, args.warmup)
    lines.append("rgba_prepare   800x800x4 identity   rows + valid_mask                (1 launch)     %8.1f / %8.1f / %8.1f" % (med, lo, hi))
    med, lo, hi = timed(lambda: ops.lanczos_resize(src3, (SIDE, SIDE), out="rows"), args.calls, args.warmup)
    lines.append("lanczos_resize 800x800x3 identity   rows                             (1 launch)     %8.1f / %8.1f / %8.1f" % (med, lo, hi))
    for side in (400, 100):
        lines.append("RGBA / three-channel at %dx%d: %.2f x plain, %.2f x with both perturbations"
                     % (side, side, medians[("rgba", side, "plain")] / medians[("rgb", side)], medians[("rgba", side, "occ + color")] / medians[("rgb", side)]))
    try:
        from PIL import Image
    except ImportError:
        lines.append("Pillow is not installed on this host: the host cost of the same preparation was not measured")
    else:
        import PIL
        lines.append("the same RGBA resizes + ToTensor + blend through Pillow %s / torch on this host (one thread), milliseconds (median / min / max of 5):" % PIL.__version__)
        for side in (400, 100):
            ts = []
            for _ in range(5):
                t0 = time.perf_counter()
                r = torch.from_numpy(np.asarray(Image.fromarray(host).resize((side, side), Image.LANCZOS))).permute(2, 0, 1).contiguous().to(torch.float32).div(255)
                r = (r[:3] * r[-1:] + (1 - r[-1:])).view(3, -1).permute(1, 0).contiguous()
                ts.append(1e3 * (time.perf_counter() - t0))
            ts.sort()
            lines.append("800x800x4 -> %dx%d   %8.2f / %8.2f / %8.2f" % (side, side, statistics.median(ts), ts[0], ts[-1]))
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()

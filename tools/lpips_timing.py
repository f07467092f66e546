"""Call time of crnerf_amd.metrics.lpips next to metrics.image_metrics (the two calls behind one result.txt line) on the GPU:
a 340 x 514 image scored on its right half with the PNG round trip, and one 800 x 800 image.  Device events around every call,
median / min / max of the steady state after a warm-up.  Gaussian weights of the network's shapes (timing does not depend on values).

    python tools/lpips_timing.py [--calls 200] [--warmup 20] [--out FILE]
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _lpips_cases as L  # noqa: E402
from crnerf_amd import _lib, metrics  # noqa: E402


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
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("lpips_timing: needs a GPU")
    dev = "cuda:0"
    wd = metrics.load_lpips_weights(L.lpips_state_dict(L.gaussian_weights(11)), device=dev)
    lib = _lib.load()
    lines = ["lpips_timing: %s, %d calls after %d warm-up calls, device events per call, microseconds (median / min / max)"
             % (torch.cuda.get_device_name(0), args.calls, args.warmup)]
    g = torch.Generator().manual_seed(0)
    for name, H, W, half, q in (("340x514, right half (257 wide), quantize_pred", 340, 514, "right", True), ("800x800, whole image", 800, 800, None, False)):
        a, b = torch.rand(1, 3, H, W, generator=g).to(dev), torch.rand(1, 3, H, W, generator=g).to(dev)
        w = W - W // 2 if half else W
        lines.append("%s   (workspace %.1f MB)" % (name, lib.crnerf_lpips_workspace_bytes(w, H) / 1e6))
        for what, fn in (("metrics.image_metrics (2 launches)", lambda: metrics.image_metrics(a, b, half=half, quantize_pred=q)),
                         ("metrics.lpips (14 launches)", lambda: metrics.lpips(a, b, wd, half=half, quantize_pred=q)),
                         ("both", lambda: (metrics.image_metrics(a, b, half=half, quantize_pred=q), metrics.lpips(a, b, wd, half=half, quantize_pred=q)))):
            med, lo, hi = timed(fn, args.calls, args.warmup)
            lines.append("    %-36s %9.1f / %9.1f / %9.1f" % (what, med, lo, hi))
        lines.append("    lpips = %.6f" % float(metrics.lpips(a, b, wd, half=half, quantize_pred=q)))
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()

"""Call time of crnerf_amd.ops.lanczos_resize on the GPU for 700 x 1000 and 1400 x 2000 photos at 1/2 (rows store, the rgbs layout) and
1/8 (signed chw store, the whole_img layout): device events around every call, median / min / max of the steady state after a
warm-up, and the bytes the passes move -- source read, uint8 intermediate written and read, output written -- over the median as a
share of the HBM rate.  Then datasets.images.build_train_buffers on 64 synthetic 700 x 1000 host photos (wall clock, synchronised), and,
where Pillow is installed, the same resizes + conversions through Pillow / torch on this host: the cost the kernel replaces.

    python tools/lanczos_timing.py [--calls 200] [--warmup 20] [--out FILE]
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

from crnerf_amd import _lib, ops  # noqa: E402
from crnerf_amd.datasets import images  # noqa: E402

HBM_PEAK = 8.0e12        # bytes/s, the MI355X data sheet


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


def moved_bytes(H, W, w, h, out_bytes_per_value):
    """Source read + intermediate written and read + output written."""
    mid = _lib.load().crnerf_lanczos_workspace_bytes(H, W, w, h)
    return H * W * 3 + 2 * mid + h * w * 3 * out_bytes_per_value


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("lanczos_timing: needs a GPU")
    dev = "cuda:0"
    rng = np.random.default_rng(0)
    lines = ["lanczos_timing: %s, %d calls after %d warm-up calls, device events per call, microseconds (median / min / max)"
             % (torch.cuda.get_device_name(0), args.calls, args.warmup)]
    cases = []
    for H, W in ((700, 1000), (1400, 2000)):
        host = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        src = torch.from_numpy(host).to(dev)
        for d, out, signed in ((2, "rows", False), (8, "chw", True)):
            w, h = W // d, H // d
            med, lo, hi = timed(lambda: ops.lanczos_resize(src, (w, h), out=out, signed=signed), args.calls, args.warmup)
            nbytes = moved_bytes(H, W, w, h, 4)
            lines.append("%4dx%-4d -> 1/%d (%s%s, 2 launches)   %8.1f / %8.1f / %8.1f    %.2f MB moved, %.1f GB/s = %.2f %% of the 8 TB/s HBM peak"
                         % (H, W, d, "signed " if signed else "", out, med, lo, hi, nbytes / 1e6, nbytes / med / 1e3, 100 * nbytes / (med * 1e-6) / HBM_PEAK))
            cases.append((host, w, h, signed))
    # the training-set build: 64 host photos in, buffers on the device out
    photos = [torch.from_numpy(rng.integers(0, 256, (700, 1000, 3), dtype=np.uint8)) for _ in range(64)]
    K = np.array([[450.0, 0, 250], [0, 450.0, 175], [0, 0, 1]], dtype=np.float32)
    c2w = np.eye(4, dtype=np.float32)[:3]
    build = lambda: images.build_train_buffers(photos, [K] * 64, [c2w] * 64, [0.1] * 64, [5.0] * 64, list(range(64)), 2)  # noqa: E731
    build()
    torch.cuda.synchronize()
    walls = []
    for _ in range(3):
        t0 = time.perf_counter()
        build()
        torch.cuda.synchronize()
        walls.append(time.perf_counter() - t0)
    lines.append("build_train_buffers, 64 host photos of 700x1000 at img_downscale 2 (upload, 2 resizes, rays per photo), wall clock of 3 runs after one: "
                 + " / ".join("%.1f ms" % (1e3 * t) for t in walls))
    try:
        from PIL import Image
    except ImportError:
        lines.append("Pillow is not installed on this host: the host cost of the same resizes was not measured")
    else:
        import PIL
        lines.append("the same resizes through Pillow %s + the torch conversions on this host (one thread), milliseconds (median / min / max of 5):" % PIL.__version__)
        for host, w, h, signed in cases:
            ts = []
            for _ in range(5):
                t0 = time.perf_counter()
                r = torch.from_numpy(np.asarray(Image.fromarray(host).resize((w, h), Image.LANCZOS))).permute(2, 0, 1).contiguous().to(torch.float32).div(255)
                r = (r - 0.5) / 0.5 if signed else r.view(3, -1).permute(1, 0).contiguous()
                ts.append(1e3 * (time.perf_counter() - t0))
            ts.sort()
            lines.append("%4dx%-4d -> %dx%d   %8.2f / %8.2f / %8.2f" % (host.shape[0], host.shape[1], h, w, statistics.median(ts), ts[0], ts[-1]))
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()

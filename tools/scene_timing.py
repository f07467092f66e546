"""Call time of crnerf_amd.ops.scene_bounds on the GPU for 1,024 images at 200,000 and at 50,000 points: device events around every call,
median / min / max of the steady state after a warm-up, the depth evaluations per second (six passes over the points per image) and the
bytes those passes read from the caches (24 B per point and pass).  Then the same bounds the reference's way -- per image one
[P, 4] x [4, 4] product, the depth > 0 filter and two np.percentile calls, datasets/phototourism_mask_grid_sample.py:133-137 -- on this
host, one thread, on the same arrays, for the first images of the set.

    python tools/scene_timing.py [--calls 50] [--warmup 5] [--host-images 16] [--out FILE]
"""
import argparse
import os
import statistics
import sys
import time

for _v in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):      # the host baseline is one thread, as the reference's loader runs
    os.environ[_v] = "1"

import numpy as np  # noqa: E402
import torch  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from crnerf_amd import ops  # noqa: E402

PASSES = 6               # csrc/scenebounds.hip: 11/11/11/10/10/10 bits
POINT_BYTES = 24


def model(seed, n_images, n_points):
    """A landmark-sized blob and cameras around and inside it: about half the points in front of a typical camera."""
    rng = np.random.default_rng(seed)
    xyz = rng.normal(0.0, 4.0, (n_points, 3))
    q = rng.normal(size=(n_images, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    w, x, y, z = q.T
    R = np.empty((n_images, 3, 3))
    R[:, 0] = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], 1)
    R[:, 1] = np.stack([2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)], 1)
    R[:, 2] = np.stack([2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], 1)
    centres = rng.normal(0.0, 3.0, (n_images, 3))
    w2c = np.zeros((n_images, 4, 4))
    w2c[:, :3, :3] = R
    w2c[:, :3, 3] = -np.einsum("nij,nj->ni", R, centres)
    w2c[:, 3, 3] = 1.0
    return xyz, w2c


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
    t = sorted(a.elapsed_time(b) for a, b in ev)
    return statistics.median(t), t[0], t[-1]


def host_loop(xyz, w2c):
    """The reference's loop body, per image: all three camera-space coordinates through one matrix product, then the two percentiles."""
    xyz_h = np.concatenate([xyz, np.ones((len(xyz), 1))], -1)
    nears, fars = [], []
    for m in w2c:
        cam = (xyz_h @ m.T)[:, :3]
        cam = cam[cam[:, 2] > 0]
        nears.append(np.percentile(cam[:, 2], 0.1))
        fars.append(np.percentile(cam[:, 2], 99.9))
    return np.array(nears), np.array(fars)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--images", type=int, default=1024)
    ap.add_argument("--host-images", type=int, default=16)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("scene_timing: needs a GPU")
    dev = "cuda:0"
    lines = ["scene_timing: %s, %d images, %d calls after %d warm-up calls, device events per call, milliseconds (median / min / max)"
             % (torch.cuda.get_device_name(0), args.images, args.calls, args.warmup)]
    host = []
    for n_points in (200000, 50000):
        xyz, w2c = model(n_points, args.images, n_points)
        x, r = torch.from_numpy(xyz).to(dev), torch.from_numpy(np.ascontiguousarray(w2c[:, 2, :])).to(dev)
        nears, fars, counts = ops.scene_bounds(x, r)
        med, lo, hi = timed(lambda: ops.scene_bounds(x, r), args.calls, args.warmup)
        evals = args.images * n_points * PASSES
        lines.append("N = %d, P = %6d: %8.3f / %8.3f / %8.3f ms   %.1f us per image, %.3g depth evaluations/s (%d passes), %.2f MB read per pass and image, "
                     "%.2f TB/s from the caches; %d ... %d points in front (mean %.0f)"
                     % (args.images, n_points, med, lo, hi, 1e3 * med / args.images, evals / (med * 1e-3), PASSES, n_points * POINT_BYTES / 1e6,
                        evals * POINT_BYTES / (med * 1e-3) / 1e12, int(counts.min()), int(counts.max()), float(counts.float().mean())))
        k = min(args.host_images, args.images)
        t0 = time.perf_counter()
        hn, hf = host_loop(xyz, w2c[:k])
        dt = time.perf_counter() - t0
        d = max(np.abs(hn - nears[:k].cpu().numpy()).max(), np.abs(hf - fars[:k].cpu().numpy()).max())
        host.append("N = %d, P = %6d: %8.2f ms per image over the first %d images = %.1f s for all %d; largest |difference| to the device bounds %.2g"
                    % (args.images, n_points, 1e3 * dt / k, k, dt / k * args.images, args.images, d))
    lines.append("the reference's numpy loop on this host (numpy %s, one thread), the same arrays:" % np.__version__)
    lines += host
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()

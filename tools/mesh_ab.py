"""Time of the mesh extraction (crnerf_mesh_count_f32 / crnerf_mesh_emit_f32, include/crnerf_mesh.h) beside the launch that made its
grid (crnerf_sigma_grid_*), and beside what its own byte count would take at the HBM rate.  One GPU, one run.

    python tools/mesh_ab.py [--steps 10] [--warmup 3] [--sizes 128,256,512] [--out FILE]

Bare ABI launches (ctypes on the loaded library) on fixed buffers, INTERLEAVED per round so that all series see the same clocks: the count call (the
count kernel and the single-workgroup scan), the emit call with normals, and the sigma_grid launch; one pair of HIP events around every member, the
first `warmup` rounds discarded, median [min .. max] of the rest -- the bracket is the run-to-run spread.  Then ops.mesh_grid as a caller sees it:
count, the read-back, two allocations, emit, under a host clock that ends in a synchronise.
Fields: a sphere (R^2 - |p|^2, threshold 0, on linspace(-1, 1, n) axes) and the density of the trained checkpoint of tests/golden/g16_trained.npz on
[-1.2, 1.2]^3 (bf16 query), cut at the 90th percentile of a 64^3 probe of the same box.
Bytes: what the passes must move if every byte crossed the memory interface once -- count: 4 N of sigma read, 5 N of workspace written, 16 per 1,024
nodes written, read and written again by the scan; emit: N mask bytes read, 24 V of vertices and normals and 12 F of faces written (the sparse reads
around the surface -- offsets, sigma and axes of the active nodes -- are not counted).  Divided by 6.3 TB/s (the achievable HBM rate of the part) this
is a floor for a grid that does not fit the 256 MiB last-level cache, and no floor at all for one that does (128^3 = 8 MiB, 256^3 = 64 MiB of sigma)."""
import argparse
import ctypes
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HBM = 6.3e12      # bytes / s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sizes", default="128,256,512")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
        if a.out:      # written as it grows: a run that is cut short leaves what it measured
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    from crnerf_amd import _lib, ops
    dev = torch.device("cuda:0")
    lib = _lib.load()
    vp = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    say("tools/mesh_ab.py   (one MI355X, one run; library %s)" % os.path.relpath(_lib.LIB_PATH, ROOT))
    say("rounds of count, emit, sigma_grid; %d timed after %d discarded; us, median [min .. max]; floor = bytes / 6.3 TB/s" % (a.steps, a.warmup))
    z = np.load(os.path.join(ROOT, "tests", "golden", "g16_trained.npz"))
    state = {k: torch.from_numpy(z["sd__nerf_coarse." + k]).to(dev) for k in ops.MLP_TENSOR_NAMES}
    packs = {p: ops.pack_mlp_weights(state, precision=p) for p in ("bf16", "f32")}
    probe_ax = torch.linspace(-1.2, 1.2, 64, device=dev)
    cut = float(torch.quantile(ops.sigma_grid(packs["bf16"], probe_ax, probe_ax, probe_ax, precision="bf16").reshape(-1)[::7].contiguous(), 0.9))

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3

    def fmt(v):
        return "%.1f [%.1f .. %.1f]" % (statistics.median(v), min(v), max(v))

    for n in [int(s) for s in a.sizes.split(",")]:
        N = n ** 3
        ax = torch.linspace(-1.0, 1.0, n, device=dev)
        bx = torch.linspace(-1.2, 1.2, n, device=dev)
        sphere = (0.49 - (ax[None, None, :] ** 2 + ax[None, :, None] ** 2 + ax[:, None, None] ** 2)).contiguous()
        trained = torch.empty(n, n, n, dtype=torch.float32, device=dev)
        s = _lib.stream_ptr()
        ws = torch.empty(lib.crnerf_mesh_workspace_bytes(n, n, n), dtype=torch.uint8, device=dev)
        counts = torch.zeros(2, dtype=torch.int64, device=dev)
        grid_precisions = ("bf16", "f32") if n <= 256 else ("bf16",)

        def grid(precision):
            _lib.check(getattr(lib, "crnerf_sigma_grid_" + precision)(vp(packs[precision]), vp(bx), vp(bx), vp(bx), n, n, n, vp(trained), s), "sigma_grid")

        grid("bf16")
        for name, sigma, axes, thr in (("sphere", sphere, ax, 0.0), ("trained", trained, bx, cut)):
            def count():
                _lib.check(lib.crnerf_mesh_count_f32(vp(sigma), n, n, n, thr, vp(ws), vp(counts), s), "mesh_count")

            count()
            V, F = counts.tolist()
            v, nr = torch.empty(V, 3, device=dev), torch.empty(V, 3, device=dev)
            f = torch.empty(F, 3, dtype=torch.int32, device=dev)

            def emit():
                _lib.check(lib.crnerf_mesh_emit_f32(vp(sigma), vp(axes), vp(axes), vp(axes), n, n, n, thr, vp(ws), V, F, vp(v), vp(nr), vp(f), s), "mesh_emit")

            series = {"count": [], "emit": [], "whole": []}
            series.update({"grid " + p: [] for p in grid_precisions})
            for i in range(a.warmup + a.steps):
                t = {"count": timed(count), "emit": timed(emit)}
                if name == "trained":      # the launch that made this grid (it rewrites the same values)
                    for p in grid_precisions[::-1]:      # bf16 last: the grid the mesh is cut from stays the bf16 one
                        t["grid " + p] = timed(lambda: grid(p))
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = ops.mesh_grid(sigma, axes, axes, axes, thr)
                torch.cuda.synchronize()
                t["whole"] = (time.perf_counter() - t0) * 1e6
                if i >= a.warmup:
                    for k, x in t.items():
                        series[k].append(x)
            same = torch.equal(out[0], v) and torch.equal(out[1], f) and torch.equal(out[2], nr)
            nb = (N + 1023) // 1024
            b_count, b_emit = 9 * N + 48 * nb, N + 24 * V + 12 * F
            fl_c, fl_e = b_count / HBM * 1e6, b_emit / HBM * 1e6
            mc, me = statistics.median(series["count"]), statistics.median(series["emit"])
            say("%-7s %3d^3 = %9d nodes, threshold %.4g: V %d F %d; ops.mesh_grid == the bare calls: %s" % (name, n, N, thr, V, F, same))
            say("    count %s  (%.1f MB, floor %.1f: reaches %.2f of it)   emit %s  (%.1f MB, floor %.1f: reaches %.2f of it)"
                % (fmt(series["count"]), b_count / 1e6, fl_c, fl_c / mc, fmt(series["emit"]), b_emit / 1e6, fl_e, fl_e / me))
            say("    count + emit %.1f (floor %.1f: %.2f)   ops.mesh_grid, host clock %s" % (mc + me, fl_c + fl_e, (fl_c + fl_e) / (mc + me), fmt(series["whole"])))
            for p in grid_precisions:
                if series["grid " + p]:
                    mg = statistics.median(series["grid " + p])
                    say("    sigma_grid %-4s %s: count + emit is %.4f of it" % (p, fmt(series["grid " + p]), (mc + me) / mg))
            del v, nr, f, out
        del sphere, trained, ws


if __name__ == "__main__":
    main()

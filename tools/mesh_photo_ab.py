"""Time of photo colours for meshes (crnerf_mesh_zbuffer_f32, crnerf_mesh_photo_colors_u8; csrc/crnerf_mesh_photo.h) beside the
route a caller had before: the mesh to the host and a NumPy projection / bilinear gather per view.  One GPU, one run.  The method is that of
tools/mesh_smooth_ab.py.

    python tools/mesh_photo_ab.py [--steps 10] [--warmup 3] [--size 256] [--views 32,128] [--out FILE]

Bare ABI calls (ctypes on the loaded library) on fixed buffers, INTERLEAVED per round so that all series see the same clocks: the z-buffer and the
colour pass (normals and the z-buffer handed over) of both meshes at every view count; one pair of HIP events around every member, the first
`warmup` rounds discarded, median [min .. max] of the rest -- the bracket is the run-to-run spread.  Each is set against what it must do:
    z-buffer   bytes   12 F N + 12 V + 8 P    the faces once a view, the vertices once (their gathers are what the caches are for), the fill and the
                                               minimum's read-modify-write of P = N W H pixels
               fp64    87 F N + 9 C           a (face, view) pair projects three corners (25 operations each, a division counted as one) and
                                               quantises them (12); a covered pixel (C of them: the atomics issued) takes 7 divisions and 2 sums
    colours    bytes   40 V + 16 K            vertices, normals, colours and counts; K = the (vertex, view) pairs that count: 12 bytes of photo and 4 of depth
               fp64    31 V N + 36 K          a (vertex, view) pair is projected and tested for facing (25 + 6); a counting one is sampled (3 x 11 + 3)
at 6.3 TB/s and at 39.3 T fp64 operations/s (the vector unit's 78.6 TFLOP/s counts a fused multiply-add as two; the rules allow none).
Then Mesh.depth_maps and Mesh.colorize_from_photos as a caller sees them, under a host clock that ends in a synchronise; and the host route --
vertices to the host, per view a float64 projection, the range test and a bilinear gather, the mean, back to the device -- WITHOUT an occlusion
test: a lower bound of what the host route costs.
Field: the density of the trained checkpoint of tests/golden/g16_trained.npz on [-1.2, 1.2]^3 (bf16 query), cut at the 90th percentile of a 64^3
probe of the same box, largest part -- the mesh of profiles/r25/mesh_smooth.txt -- and its simplify() at 2 grid spacings.  Views: N synthetic
400 x 300 pinhole cameras on three rings around the mesh's centre, looking at it, the mesh about 0.8 of the frame's height; photos: seeded noise."""
import argparse
import ctypes
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HBM = 6.3e12      # bytes / s
F64 = 39.3e12     # operations / s without fused multiply-adds
W, H = 400, 300


def ring_views(np, centre, radius, n):
    """n cameras on three rings (elevations -25, 10, 45 degrees) at 3 radii from the centre, looking at it."""
    Ks, poses = [], []
    focal = 0.8 * (H / 2) * 3.0          # a sphere of `radius` at 3 radii fills about 0.8 of the height
    for k in range(n):
        az = 2 * math.pi * k / n + 0.1
        el = math.radians((-25.0, 10.0, 45.0)[k % 3])
        eye = centre + 3.0 * radius * np.array([math.cos(el) * math.cos(az), math.cos(el) * math.sin(az), math.sin(el)])
        back = (eye - centre) / np.linalg.norm(eye - centre)
        right = np.cross([0.0, 0.0, 1.0], back)
        right /= np.linalg.norm(right)
        poses.append(np.stack((right, np.cross(back, right), back, eye), axis=1))
        Ks.append([[focal, 0, (W - 1) / 2], [0, focal, (H - 1) / 2], [0, 0, 1]])
    return np.array(Ks), np.stack(poses)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--views", default="32,128")
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
    from crnerf_amd import _lib, geometry, ops
    dev = torch.device("cuda:0")
    lib = _lib.load()
    vp = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    counts = [int(s) for s in a.views.split(",")]
    say("tools/mesh_photo_ab.py   (one MI355X, one run; library %s)" % os.path.relpath(_lib.LIB_PATH, ROOT))
    say("rounds of z-buffer and colours (both meshes, %s views of %d x %d); %d timed after %d discarded; us, median [min .. max]"
        % (" and ".join(str(c) for c in counts), W, H, a.steps, a.warmup))
    z = np.load(os.path.join(ROOT, "tests", "golden", "g16_trained.npz"))
    state = {k: torch.from_numpy(z["sd__nerf_coarse." + k]).to(dev) for k in ops.MLP_TENSOR_NAMES}
    pack = ops.pack_mlp_weights(state, precision="bf16")
    probe_ax = torch.linspace(-1.2, 1.2, 64, device=dev)
    cut = float(torch.quantile(ops.sigma_grid(pack, probe_ax, probe_ax, probe_ax, precision="bf16").reshape(-1)[::7].contiguous(), 0.9))
    n = a.size
    bx = torch.linspace(-1.2, 1.2, n, device=dev)
    full = geometry.DensityGrid(ops.sigma_grid(pack, bx, bx, bx, precision="bf16"), bx, bx, bx).mesh(cut).largest()
    small = full.simplify(2 * 2.4 / (n - 1), lo=(-1.2, -1.2, -1.2), hi=(1.2, 1.2, 1.2)).recompute_normals()
    box = torch.stack((full.vertices.min(dim=0).values, full.vertices.max(dim=0).values)).cpu().numpy().astype(np.float64)
    centre, radius = box.mean(axis=0), float(np.linalg.norm(box[1] - box[0]) / 2)
    say("trained %d^3, threshold %.4g; centre %s, radius %.3f" % (n, cut, np.round(centre, 3).tolist(), radius))
    s = _lib.stream_ptr()

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3

    def fmt(v):
        return "%.1f [%.1f .. %.1f]" % (statistics.median(v), min(v), max(v))

    def share(us, nbytes, nops):
        tb, to = nbytes / HBM * 1e6, nops / F64 * 1e6
        return ("%.1f MB = %.1f us at 6.3 TB/s, %.2f G fp64 operations = %.1f us at 39.3 T/s: %.2f of the larger (%s)"
                % (nbytes / 1e6, tb, nops / 1e9, to, max(tb, to) / us, "bytes" if tb > to else "fp64"))

    members, cases = [], {}
    for N in counts:
        Ks, poses = ring_views(np, centre, radius, N)
        views = geometry.Views(Ks, poses, [(W, H)] * N)
        photos = torch.from_numpy(np.random.default_rng(N).integers(0, 256, (views.total_pixels, 3), dtype=np.uint8)).to(dev)
        for tag, mesh in (("extracted", full), ("simplified", small)):
            v, f, nrm = mesh.vertices, mesh.faces, mesh.normals
            V, F, P = v.shape[0], f.shape[0], views.total_pixels
            depth = torch.empty(P, dtype=torch.float32, device=dev)
            colors, seen = torch.empty(V, 3, device=dev), torch.empty(V, dtype=torch.int32, device=dev)

            def zbuffer(v=v, f=f, V=V, F=F, views=views, N=N, P=P, depth=depth):
                _lib.check(lib.crnerf_mesh_zbuffer_f32(vp(v), vp(f), V, F, vp(views.cams), vp(views.dims), vp(views.offset_table), N, P, 1e-3, vp(depth), s), "zbuffer")

            def colour(v=v, nrm=nrm, V=V, photos=photos, views=views, N=N, P=P, depth=depth, colors=colors, seen=seen):
                _lib.check(lib.crnerf_mesh_photo_colors_u8(vp(v), vp(nrm), V, vp(photos), vp(depth), vp(views.cams), vp(views.dims), vp(views.offset_table), N, P,
                                                           1e-3, 0.02, vp(colors), vp(seen), s), "colours")

            zbuffer()
            colour()
            key = "%s, %d views" % (tag, N)
            members += [("zbuffer " + key, zbuffer), ("colours " + key, colour)]
            cases[key] = (mesh, views, photos, V, F, N, P, int(torch.isfinite(depth).sum()), int(seen.sum()), int((seen > 0).sum()))
    series = {name: [] for name, _ in members}
    for key in cases:
        series["depth_maps " + key], series["colorize " + key] = [], []
    for i in range(a.warmup + a.steps):
        t = {name: timed(fn) for name, fn in members}
        for key, (mesh, views, photos, *_rest) in cases.items():
            for name, call in (("depth_maps ", lambda: mesh.depth_maps(views)), ("colorize ", lambda: mesh.colorize_from_photos(photos, views))):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                got = call()
                torch.cuda.synchronize()
                t[name + key] = (time.perf_counter() - t0) * 1e6
        if i >= a.warmup:
            for name, x in t.items():
                series[name].append(x)
    del got
    med = {name: statistics.median(x) for name, x in series.items()}
    for key, (mesh, views, photos, V, F, N, P, covered, K, coloured) in cases.items():
        say("  %s: V %d F %d, %d pixels of which %d covered; %d (vertex, view) pairs count, %d vertices coloured" % (key, V, F, P, covered, K, coloured))
        # the atomics issued are not counted by the kernel: the covered pixels are their lower bound, and what the figure below uses
        say("    z-buffer %s   %s" % (fmt(series["zbuffer " + key]), share(med["zbuffer " + key], 12 * F * N + 12 * V + 8 * P, 87 * F * N + 9 * covered)))
        say("    colours %s   %s" % (fmt(series["colours " + key]), share(med["colours " + key], 40 * V + 16 * K, 31 * V * N + 36 * K)))
        say("    Mesh.depth_maps, host clock %s;   Mesh.colorize_from_photos (z-buffer, colours, fallback), host clock %s"
            % (fmt(series["depth_maps " + key]), fmt(series["colorize " + key])))
        host = []
        photos_h = photos.cpu().numpy().reshape(N, H, W, 3)
        cams = views.cams.cpu().numpy()
        for _ in range(3 if V < 200000 or N <= 32 else 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            x = mesh.vertices.cpu().numpy().astype(np.float64)
            t1 = time.perf_counter()
            acc, cnt = np.zeros((V, 3)), np.zeros(V)
            for k in range(N):
                fx, fy, cx, cy = cams[k, :4]
                c = (x - cams[k, 13:16]) @ cams[k, 4:13].reshape(3, 3)
                zc = -c[:, 2]
                with np.errstate(all="ignore"):
                    u, w = cx + fx * (c[:, 0] / zc), cy - fy * (c[:, 1] / zc)
                    ok = np.nonzero((zc >= 1e-3) & (u >= 0) & (u <= W - 1) & (w >= 0) & (w <= H - 1))[0]
                u, w = u[ok], w[ok]
                x0, y0 = np.minimum(np.floor(u).astype(np.int64), W - 2), np.minimum(np.floor(w).astype(np.int64), H - 2)
                fa, fb = (u - x0)[:, None], (w - y0)[:, None]
                img = photos_h[k]
                top = img[y0, x0] * (1 - fa) + img[y0, x0 + 1] * fa
                bot = img[y0 + 1, x0] * (1 - fa) + img[y0 + 1, x0 + 1] * fa
                acc[ok] += top * (1 - fb) + bot * fb
                cnt[ok] += 1
            t2 = time.perf_counter()
            back = torch.from_numpy((acc / np.maximum(cnt, 1)[:, None] / 255.0).astype(np.float32)).to(dev)
            torch.cuda.synchronize()
            t3 = time.perf_counter()
            host.append(((t3 - t0) * 1e3, (t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3))
        best = sorted(host)[len(host) // 2]
        free, _ = geometry.photo_colors(mesh.vertices, photos, views)      # no normals, no z-buffer: what the host route computes
        say("    on the host instead, no occlusion test (NumPy): %.1f ms (to the host %.1f, %d views %.1f, back %.1f; median of %d);  "
            "largest |colour - device's, nothing tested| %.3g" % (best[0], best[1], N, best[2], best[3], len(host), float((back - free).abs().max())))
        del back, free, photos_h


if __name__ == "__main__":
    main()

"""Time of mesh smoothing and face normals (crnerf_mesh_adjacency_i32, crnerf_mesh_smooth_f32, crnerf_mesh_vertex_normals_f32;
csrc/crnerf_mesh_smooth.h) beside the same smoothing done on the host, and beside the launch that made the grid.  One GPU, one
run.  The method is that of tools/mesh_parts_ab.py and tools/mesh_simplify_ab.py.

    python tools/mesh_smooth_ab.py [--steps 10] [--warmup 3] [--sizes 256,512] [--out FILE]

Bare ABI calls (ctypes on the loaded library) on fixed buffers, INTERLEAVED per round so that all series see the same clocks: the adjacency, smooth
with 0 steps (quantise and write out) and with 10 (20 passes more: one pass = the difference / 20), the normals, and the bf16 sigma_grid launch; one
pair of HIP events around every member, the first `warmup` rounds discarded, median [min .. max] of the rest -- the bracket is the run-to-run
spread.  Each is set against the bytes it must move, at 6.3 TB/s:
    adjacency   48 F + 28 V    the faces twice (degree, fill), the neighbour list written, deg / cursor / h zeroed, deg read and the row starts written
    one pass    40 V + 24 F    P read and written (16 bytes a vertex: the row's length rides in the fourth word), the row start of every vertex, the
                               neighbour list; the gathered P (96 F bytes if every entry missed) is not counted: it is what the caches are for
    normals     12 F + 72 V    the faces, the sums zeroed, added to, read, the normals written; the gathered vertices are not counted
Then Mesh.smooth(10) as a caller sees it (the bounding-box read-back, the workspaces, adjacency, 20 passes, normals) under a host clock that ends in
a synchronise; and what a user of the parent commit does instead -- the mesh to the host, a scipy.sparse neighbour-count matrix (np.add.at where
scipy is missing), 20 float64 passes, back to the device.
Field: the density of the trained checkpoint of tests/golden/g16_trained.npz on [-1.2, 1.2]^3 (bf16 query), cut at the 90th percentile of a 64^3
probe of the same box, largest part -- the mesh of profiles/r21/mesh.txt, r22/mesh_parts.txt and r24/mesh_simplify.txt -- and its simplify() at
2 grid spacings."""
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
    ap.add_argument("--sizes", default="256,512")
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
    try:
        import scipy.sparse as sparse
    except ImportError:
        sparse = None
    dev = torch.device("cuda:0")
    lib = _lib.load()
    vp = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    say("tools/mesh_smooth_ab.py   (one MI355X, one run; library %s)" % os.path.relpath(_lib.LIB_PATH, ROOT))
    say("rounds of adjacency, smooth 0 steps, smooth 10 steps, vertex normals (both meshes), sigma_grid bf16; %d timed after %d discarded; "
        "us, median [min .. max]" % (a.steps, a.warmup))
    z = np.load(os.path.join(ROOT, "tests", "golden", "g16_trained.npz"))
    state = {k: torch.from_numpy(z["sd__nerf_coarse." + k]).to(dev) for k in ops.MLP_TENSOR_NAMES}
    pack = ops.pack_mlp_weights(state, precision="bf16")
    probe_ax = torch.linspace(-1.2, 1.2, 64, device=dev)
    cut = float(torch.quantile(ops.sigma_grid(pack, probe_ax, probe_ax, probe_ax, precision="bf16").reshape(-1)[::7].contiguous(), 0.9))

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3

    def fmt(v):
        return "%.1f [%.1f .. %.1f]" % (statistics.median(v), min(v), max(v))

    def share(us, nbytes):
        return "%.1f MB = %.1f us at 6.3 TB/s: %.2f of it" % (nbytes / 1e6, nbytes / HBM * 1e6, nbytes / HBM * 1e6 / us)

    for n in [int(s) for s in a.sizes.split(",")]:
        bx = torch.linspace(-1.2, 1.2, n, device=dev)
        sigma = torch.empty(n, n, n, dtype=torch.float32, device=dev)
        s = _lib.stream_ptr()

        def grid():
            _lib.check(lib.crnerf_sigma_grid_bf16(vp(pack), vp(bx), vp(bx), vp(bx), n, n, n, vp(sigma), s), "sigma_grid")

        grid()
        full = geometry.DensityGrid(sigma, bx, bx, bx).mesh(cut).largest()
        small = full.simplify(2 * 2.4 / (n - 1), lo=(-1.2, -1.2, -1.2), hi=(1.2, 1.2, 1.2))
        members, meshes = [("grid bf16", grid)], {}
        for tag, mesh in (("extracted", full), ("simplified", small)):
            v, f = mesh.vertices, mesh.faces
            V, F = v.shape[0], f.shape[0]
            lo, e = geometry._lattice_box(v, "mesh_smooth_ab")
            lo = [ctypes.c_float(x).value for x in lo]
            ws = torch.empty(lib.crnerf_mesh_smooth_workspace_bytes(V, F), dtype=torch.uint8, device=dev)
            out, nrm = torch.empty_like(v), torch.empty_like(v)

            def adjacency(f=f, V=V, F=F, ws=ws):
                _lib.check(lib.crnerf_mesh_adjacency_i32(vp(f), V, F, vp(ws), s), "adjacency")

            def smooth(steps, v=v, V=V, F=F, lo=lo, e=e, ws=ws, out=out):
                _lib.check(lib.crnerf_mesh_smooth_f32(vp(v), V, F, *lo, 29 - e, steps, 0.5, -0.53, 1, vp(ws), vp(out), s), "smooth")

            def normals(f=f, V=V, F=F, e=e, ws=ws, out=out, nrm=nrm):
                _lib.check(lib.crnerf_mesh_vertex_normals_f32(vp(out), vp(f), V, F, 44 - 2 * e, vp(ws), vp(nrm), s), "normals")

            adjacency()
            members += [("adjacency " + tag, adjacency), ("smooth0 " + tag, lambda smooth=smooth: smooth(0)), ("smooth10 " + tag, lambda smooth=smooth: smooth(10)),
                        ("normals " + tag, normals)]
            meshes[tag] = (mesh, V, F, ws.numel(), out)
        series = {name: [] for name, _ in members}
        for tag in meshes:
            series["Mesh.smooth " + tag] = []
        for i in range(a.warmup + a.steps):
            t = {name: timed(fn) for name, fn in members}
            for tag, (mesh, *_rest) in meshes.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                got = mesh.smooth(10)
                torch.cuda.synchronize()
                t["Mesh.smooth " + tag] = (time.perf_counter() - t0) * 1e6
            if i >= a.warmup:
                for name, x in t.items():
                    series[name].append(x)
        med = {name: statistics.median(x) for name, x in series.items()}
        say("trained %3d^3, threshold %.4g;   sigma_grid bf16 %s" % (n, cut, fmt(series["grid bf16"])))
        for tag, (mesh, V, F, wbytes, out) in meshes.items():
            one = (med["smooth10 " + tag] - med["smooth0 " + tag]) / 20.0
            call = med["adjacency " + tag] + med["smooth10 " + tag] + med["normals " + tag]
            say("  %s, largest part: V %d F %d, workspace %.0f MB" % (tag, V, F, wbytes / 1e6))
            say("    adjacency %s   %s" % (fmt(series["adjacency " + tag]), share(med["adjacency " + tag], 48 * F + 28 * V)))
            say("    smooth, 0 steps %s   10 steps %s   one pass %.1f   %s" % (fmt(series["smooth0 " + tag]), fmt(series["smooth10 " + tag]), one,
                                                                              share(one, 40 * V + 24 * F)))
            say("    normals %s   %s" % (fmt(series["normals " + tag]), share(med["normals " + tag], 12 * F + 72 * V)))
            say("    adjacency + 10 steps + normals %.1f = %.4f of the sigma_grid bf16 launch;   Mesh.smooth(10), host clock %s"
                % (call, call / med["grid bf16"], fmt(series["Mesh.smooth " + tag])))
            host = []
            for _ in range(3):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                hv, hf = mesh.vertices.cpu().numpy().astype(np.float64), mesh.faces.cpu().numpy().astype(np.int64)
                t1 = time.perf_counter()
                rows = np.concatenate([hf[:, 0], hf[:, 0], hf[:, 1], hf[:, 1], hf[:, 2], hf[:, 2]])
                cols = np.concatenate([hf[:, 1], hf[:, 2], hf[:, 2], hf[:, 0], hf[:, 0], hf[:, 1]])
                deg = np.bincount(rows, minlength=V).astype(np.float64)
                if sparse is not None:
                    A = sparse.csr_matrix((np.ones(len(rows)), (rows, cols)), shape=(V, V))      # duplicates are summed: the multiplicities
                moves = deg > 0
                t2 = time.perf_counter()
                p = hv.copy()
                for k in range(20):
                    if sparse is not None:
                        S = A @ p
                    else:
                        S = np.zeros_like(p)
                        np.add.at(S, rows, p[cols])
                    w = 0.5 if k % 2 == 0 else -0.53
                    p[moves] += w * (S[moves] / deg[moves, None] - p[moves])
                t3 = time.perf_counter()
                back = torch.from_numpy(p.astype(np.float32)).to(dev)
                torch.cuda.synchronize()
                t4 = time.perf_counter()
                host.append(((t4 - t0) * 1e3, (t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3, (t4 - t3) * 1e3))
            best = sorted(host)[1]
            lo, e = geometry._lattice_box(mesh.vertices, "mesh_smooth_ab")      # the host route pins nothing: compare with the device's unpinned result
            free = ops.mesh_smooth(mesh.vertices, mesh.faces, lo, 29 - e, 10, 0.5, -0.53, pin_border=False)
            say("    on the host instead (%s): %.1f ms (to the host %.1f, the matrix %.1f, 20 passes %.1f, back %.1f; median of 3);  "
                "largest |position - device's, nothing pinned| %.3g" % (("scipy.sparse" if sparse is not None else "np.add.at",) + best
                                                                        + (float((back - free).abs().max()),)))
            del back, free, hv, hf, rows, cols
        del got, meshes, members, full, small, sigma


if __name__ == "__main__":
    main()

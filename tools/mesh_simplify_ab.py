"""Time of the mesh simplification (crnerf_mesh_cluster_*, csrc/crnerf_mesh_simplify.h) beside the same clustering done on the host
with NumPy, and beside the launch that made the grid.  One GPU, one run.  The method is that of tools/mesh_parts_ab.py.

    python tools/mesh_simplify_ab.py [--steps 10] [--warmup 3] [--sizes 256,512] [--spacings 2,4,8] [--out FILE]

Bare ABI calls (ctypes on the loaded library) on fixed buffers, INTERLEAVED per round so that all series see the same clocks: count and emit of the
clustering at every cell size, and the bf16 sigma_grid launch; one pair of HIP events around every member, the first `warmup` rounds discarded,
median [min .. max] of the rest -- the bracket is the run-to-run spread.  Then Mesh.simplify() as a caller sees it (count, read-back of V' and F',
allocations, emit; the box is given, so there is no bounding-box read-back) under a host clock that ends in a synchronise; and what a user of the
parent commit does instead -- the mesh to the host, np.unique on the cell keys and on the sorted triples, np.add.at for the sums -- on the same
box (float64 means, not the header's fixed point: the yardstick is the work, not the bytes).
Field: the density of the trained checkpoint of tests/golden/g16_trained.npz on [-1.2, 1.2]^3 (bf16 query), cut at the 90th percentile of a 64^3
probe of the same box, largest part: the mesh of profiles/r21/mesh.txt and profiles/r22/mesh_parts.txt.  The mesh carries normals and colours
(the normals stand in as colours: their values do not change the work)."""
import argparse
import ctypes
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sizes", default="256,512")
    ap.add_argument("--spacings", default="2,4,8")
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
    say("tools/mesh_simplify_ab.py   (one MI355X, one run; library %s)" % os.path.relpath(_lib.LIB_PATH, ROOT))
    say("rounds of cluster count, cluster emit (every cell size), sigma_grid bf16; %d timed after %d discarded; us, median [min .. max]" % (a.steps, a.warmup))
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

    for n in [int(s) for s in a.sizes.split(",")]:
        bx = torch.linspace(-1.2, 1.2, n, device=dev)
        sigma = torch.empty(n, n, n, dtype=torch.float32, device=dev)
        s = _lib.stream_ptr()

        def grid():
            _lib.check(lib.crnerf_sigma_grid_bf16(vp(pack), vp(bx), vp(bx), vp(bx), n, n, n, vp(sigma), s), "sigma_grid")

        grid()
        mesh = geometry.DensityGrid(sigma, bx, bx, bx).mesh(cut).largest()
        mesh = geometry.Mesh(mesh.vertices, mesh.faces, mesh.normals, mesh.normals.abs().contiguous())
        V, F = mesh.vertices.shape[0], mesh.faces.shape[0]
        v, f, nr, col = mesh.vertices, mesh.faces, mesh.normals, mesh.colors
        spacing = 2.4 / (n - 1)
        members, state_of = [("grid bf16", grid)], {}
        for k in [int(x) for x in a.spacings.split(",")]:
            cell = k * spacing
            cells = max(1, -(-(n - 1) // k))
            g = (-1.2, -1.2, -1.2, cell, cell, cell, cells, cells, cells)
            ws = torch.empty(lib.crnerf_mesh_cluster_workspace_bytes(V, F, cells ** 3), dtype=torch.uint8, device=dev)
            vc = torch.empty(V, dtype=torch.int32, device=dev)
            counts = torch.zeros(2, dtype=torch.int64, device=dev)

            def count(g=g, ws=ws, vc=vc, counts=counts):
                _lib.check(lib.crnerf_mesh_cluster_count_f32(vp(v), vp(f), V, F, *g, vp(ws), vp(vc), vp(counts), s), "cluster_count")

            count()
            Vk, Fk = counts.tolist()
            ov, on, oc = (torch.empty(Vk, 3, device=dev) for _ in range(3))
            of = torch.empty(Fk, 3, dtype=torch.int32, device=dev)

            def emit(g=g, ws=ws, vc=vc, ov=ov, on=on, oc=oc, of=of, Vk=Vk, Fk=Fk):
                _lib.check(lib.crnerf_mesh_cluster_emit_f32(vp(v), vp(nr), vp(col), vp(f), vp(vc), V, F, *g, vp(ws), Vk, Fk, vp(ov), vp(on), vp(oc), vp(of), s),
                           "cluster_emit")

            emit()
            members += [("count %d" % k, count), ("emit %d" % k, emit)]
            state_of[k] = (cell, cells, Vk, Fk, ov, of, ws.numel())
        series = {name: [] for name, _ in members}
        for k in state_of:
            series["simplify %d" % k] = []
        for i in range(a.warmup + a.steps):
            t = {name: timed(fn) for name, fn in members}
            for k, (cell, cells, *_rest) in state_of.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = mesh.simplify(cell, lo=(-1.2, -1.2, -1.2), hi=(-1.2 + cells * cell,) * 3)
                torch.cuda.synchronize()
                t["simplify %d" % k] = (time.perf_counter() - t0) * 1e6
            if i >= a.warmup:
                for name, x in t.items():
                    series[name].append(x)
        med = {name: statistics.median(x) for name, x in series.items()}
        say("trained %3d^3, threshold %.4g, largest part: V %d F %d;   sigma_grid bf16 %s" % (n, cut, V, F, fmt(series["grid bf16"])))
        hv, hf, hn, hc = None, None, None, None
        for k, (cell, cells, Vk, Fk, ov, of, wbytes) in state_of.items():
            both = med["count %d" % k] + med["emit %d" % k]
            say("  cell = %d spacings (%d^3 cells, workspace %.0f MB): V' %d F' %d  (V / %.1f, F / %.1f)" % (k, cells, wbytes / 1e6, Vk, Fk, V / Vk, F / max(Fk, 1)))
            say("    count %s   emit %s   both %.1f = %.4f of the sigma_grid bf16 launch" % (fmt(series["count %d" % k]), fmt(series["emit %d" % k]), both,
                                                                                            both / med["grid bf16"]))
            say("    Mesh.simplify(), host clock %s" % fmt(series["simplify %d" % k]))
            host = []
            for _ in range(3):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                hv, hf, hn, hc = v.cpu().numpy(), f.cpu().numpy(), nr.cpu().numpy(), col.cpu().numpy()
                t1 = time.perf_counter()
                c = np.minimum(((hv - np.float32(-1.2)) * (np.float32(1.0) / np.float32(cell))).astype(np.int64), cells - 1)
                key = c[:, 0] + cells * (c[:, 1] + cells * c[:, 2])
                _, first, inverse = np.unique(key, return_index=True, return_inverse=True)
                rank = np.empty(len(first), np.int64)
                rank[np.argsort(first, kind="stable")] = np.arange(len(first))
                vc_h = rank[inverse.reshape(-1)]
                sums = np.zeros((len(first), 9))
                np.add.at(sums, vc_h, np.concatenate([hv, hn, hc], axis=1))
                m = np.bincount(vc_h, minlength=len(first))[:, None]
                pos, colm = sums[:, :3] / m, sums[:, 6:] / m
                nrm = sums[:, 3:6] / np.maximum(np.linalg.norm(sums[:, 3:6], axis=1, keepdims=True), 1e-30)
                t2 = time.perf_counter()
                tri = vc_h[hf]
                alive = (tri[:, 0] != tri[:, 1]) & (tri[:, 0] != tri[:, 2]) & (tri[:, 1] != tri[:, 2])
                idx = np.nonzero(alive)[0]
                _, keep = np.unique(np.sort(tri[idx], axis=1), axis=0, return_index=True)
                out_f = tri[np.sort(idx[keep])]
                t3 = time.perf_counter()
                host.append(((t3 - t0) * 1e3, (t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3))
            best = sorted(host)[1]
            agree = len(pos) == Vk and len(out_f) == Fk and np.array_equal(np.sort(out_f, axis=1), np.sort(of.cpu().numpy(), axis=1))
            say("    on the host instead: %.1f ms (to the host %.1f, vertices: np.unique + np.add.at %.1f, faces: np.unique on the triples %.1f; median of 3); "
                "same V', F' and face sets: %s;  largest |position - device's| %.3g, %.3g of a cell"
                % (best + (agree, float(np.abs(pos - ov.cpu().numpy()).max()), float(np.abs(pos - ov.cpu().numpy()).max()) / cell)))
            del pos, colm, nrm
        del out, mesh, sigma, v, f, nr, col, state_of, members


if __name__ == "__main__":
    main()

"""Time of the mesh parts (crnerf_mesh_parts_*, include/crnerf_mesh_parts.h) beside the extraction that made the mesh
(crnerf_mesh_count_f32 + crnerf_mesh_emit_f32), beside what its own byte count would take at the HBM rate, and beside the launch that made the grid.
One GPU, one run.  The method is that of tools/mesh_ab.py.

    python tools/mesh_parts_ab.py [--steps 10] [--warmup 3] [--sizes 128,256,512] [--out FILE]

Bare ABI launches (ctypes on the loaded library) on fixed buffers, INTERLEAVED per round so that all series see the same clocks: label, sizes,
select_count and select_emit (keep = the largest part), the count + emit pair of the extraction, and the bf16 sigma_grid launch; one pair of HIP events
around every member, the first `warmup` rounds discarded, median [min .. max] of the rest -- the bracket is the run-to-run spread.  Then
Mesh.largest() as a caller sees it (label, read-back of K, sizes, the ranking in torch, select_count, read-back, allocations, select_emit) under a
host clock that ends in a synchronise; and what a user of the parent commit does instead -- the mesh to the host,
scipy.sparse.csgraph.connected_components, NumPy compaction -- on the same box, when scipy imports (the line is left out otherwise).
Field: the density of the trained checkpoint of tests/golden/g16_trained.npz on [-1.2, 1.2]^3 (bf16 query), cut at the 90th percentile of a 64^3
probe of the same box: the grid of profiles/r21/mesh.txt.
Bytes: what the passes must move if every byte crossed the memory interface once -- label: the faces read twice and face_part written (28 F), parent
written, read by the union, read and written by the flatten with its 16-bit ranks, read with them by the apply, vertex_part written (30 V); the
union's finds beyond the first read of every entry, and the apply's gathers, are not counted.  sizes: 4 V + 4 F.  select_count: 6 V + 6 F.
select_emit: 6 V + 6 F of labels and offsets, 48 V' + 24 F' of rows read and written (the gathers of the remap are not counted).  Divided by
6.3 TB/s this is a floor for a mesh that does not fit the 256 MiB last-level cache, and no floor at all for one that does."""
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
    from crnerf_amd import _lib, geometry, ops
    dev = torch.device("cuda:0")
    lib = _lib.load()
    vp = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    say("tools/mesh_parts_ab.py   (one MI355X, one run; library %s)" % os.path.relpath(_lib.LIB_PATH, ROOT))
    say("rounds of label, sizes, select_count, select_emit, mesh count + emit, sigma_grid bf16; %d timed after %d discarded; us, median [min .. max]; "
        "floor = bytes / 6.3 TB/s" % (a.steps, a.warmup))
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
        mws = torch.empty(lib.crnerf_mesh_workspace_bytes(n, n, n), dtype=torch.uint8, device=dev)
        counts = torch.zeros(2, dtype=torch.int64, device=dev)

        def mesh_count():
            _lib.check(lib.crnerf_mesh_count_f32(vp(sigma), n, n, n, cut, vp(mws), vp(counts), s), "mesh_count")

        mesh_count()
        V, F = counts.tolist()
        v, nr = torch.empty(V, 3, device=dev), torch.empty(V, 3, device=dev)
        f = torch.empty(F, 3, dtype=torch.int32, device=dev)

        def mesh_emit():
            _lib.check(lib.crnerf_mesh_emit_f32(vp(sigma), vp(bx), vp(bx), vp(bx), n, n, n, cut, vp(mws), V, F, vp(v), vp(nr), vp(f), s), "mesh_emit")

        mesh_emit()
        ws = torch.empty(lib.crnerf_mesh_parts_workspace_bytes(V, F), dtype=torch.uint8, device=dev)
        vpart, fpart = torch.empty(V, dtype=torch.int32, device=dev), torch.empty(F, dtype=torch.int32, device=dev)
        kc = torch.zeros(1, dtype=torch.int64, device=dev)

        def label():
            _lib.check(lib.crnerf_mesh_parts_label_i32(vp(f), V, F, vp(ws), vp(vpart), vp(fpart), vp(kc), s), "label")

        label()
        K = int(kc.item())
        pv, pf = torch.empty(K, dtype=torch.int32, device=dev), torch.empty(K, dtype=torch.int32, device=dev)

        def sizes():
            _lib.check(lib.crnerf_mesh_parts_sizes_i32(vp(vpart), vp(fpart), V, F, K, vp(pv), vp(pf), s), "sizes")

        sizes()
        keep = torch.zeros(K, dtype=torch.uint8, device=dev)
        keep[torch.sort(pf, descending=True, stable=True).indices[:1]] = 1
        sc = torch.zeros(2, dtype=torch.int64, device=dev)
        sws = torch.empty_like(ws)      # a workspace of its own: label's is scratch, select_emit reads what select_count left

        def select_count():
            _lib.check(lib.crnerf_mesh_parts_select_count(vp(vpart), vp(fpart), V, F, K, vp(keep), vp(sws), vp(sc), s), "select_count")

        select_count()
        Vk, Fk = sc.tolist()
        ov, on = torch.empty(Vk, 3, device=dev), torch.empty(Vk, 3, device=dev)
        of = torch.empty(Fk, 3, dtype=torch.int32, device=dev)

        def select_emit():
            _lib.check(lib.crnerf_mesh_parts_select_emit_f32(vp(v), vp(nr), vp(f), vp(vpart), vp(fpart), V, F, K, vp(keep), vp(sws), Vk, Fk, vp(ov), vp(on),
                                                             vp(of), s), "select_emit")

        mesh = geometry.Mesh(v, f, nr)
        members = (("label", label), ("sizes", sizes), ("select_count", select_count), ("select_emit", select_emit), ("mesh count", mesh_count),
                   ("mesh emit", mesh_emit), ("grid bf16", grid))
        series = {k: [] for k, _ in members}
        series["largest"] = []
        for i in range(a.warmup + a.steps):
            t = {k: timed(fn) for k, fn in members}
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = mesh.largest()
            torch.cuda.synchronize()
            t["largest"] = (time.perf_counter() - t0) * 1e6
            if i >= a.warmup:
                for k, x in t.items():
                    series[k].append(x)
        same = torch.equal(out.vertices, ov) and torch.equal(out.faces, of) and torch.equal(out.normals, on)
        med = {k: statistics.median(x) for k, x in series.items()}
        pair = med["mesh count"] + med["mesh emit"]
        say("trained %3d^3, threshold %.4g: V %d F %d K %d; largest part V' %d F' %d; Mesh.largest() == the bare calls: %s" % (n, cut, V, F, K, Vk, Fk, same))
        say("    mesh count + emit %.1f   sigma_grid bf16 %s" % (pair, fmt(series["grid bf16"])))
        byts = {"label": 28 * F + 30 * V, "sizes": 4 * V + 4 * F, "select_count": 6 * V + 6 * F, "select_emit": 6 * V + 6 * F + 48 * Vk + 24 * Fk}
        for k in ("label", "sizes", "select_count", "select_emit"):
            fl = byts[k] / HBM * 1e6
            say("    %-12s %s  = %.2f of count + emit   (%.1f MB, floor %.1f: reaches %.2f of it)" % (k, fmt(series[k]), med[k] / pair, byts[k] / 1e6, fl, fl / med[k]))
        whole = med["label"] + med["sizes"] + med["select_count"] + med["select_emit"]
        say("    all four %.1f = %.2f of count + emit, %.4f of the sigma_grid bf16 launch;  label + select %.1f = %.4f of it"
            % (whole, whole / pair, whole / med["grid bf16"], whole - med["sizes"], (whole - med["sizes"]) / med["grid bf16"]))
        say("    Mesh.largest(), host clock %s" % fmt(series["largest"]))
        try:
            from scipy.sparse import coo_matrix
            from scipy.sparse.csgraph import connected_components
        except ImportError:
            connected_components = None
        if connected_components is not None:
            host = []
            for _ in range(3):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                hv, hf, hn = v.cpu().numpy(), f.cpu().numpy(), nr.cpu().numpy()
                t1 = time.perf_counter()
                rows, cols = np.concatenate([hf[:, 0], hf[:, 0]]), np.concatenate([hf[:, 1], hf[:, 2]])
                k, lab = connected_components(coo_matrix((np.ones(len(rows), np.int8), (rows, cols)), shape=(V, V)), directed=False)
                t2 = time.perf_counter()
                big = np.argmax(np.bincount(lab[hf[:, 0]], minlength=k))
                kv = lab == big
                new_id = np.cumsum(kv) - 1
                cv, cn, cf = hv[kv], hn[kv], new_id[hf[kv[hf[:, 0]]]].astype(np.int32)
                t3 = time.perf_counter()
                host.append(((t3 - t0) * 1e3, (t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3))
            best = sorted(host)[1]
            agree = k == K and np.array_equal(cv, ov.cpu().numpy()) and np.array_equal(cf, of.cpu().numpy()) and np.array_equal(cn, on.cpu().numpy())
            say("    on the host instead: %.1f ms (to the host %.1f, scipy connected_components %.1f, NumPy compaction %.1f; median of 3); same mesh: %s"
                % (best + (agree,)))
        del v, nr, f, ws, sws, vpart, fpart, ov, on, of, out, mesh, sigma, mws


if __name__ == "__main__":
    main()

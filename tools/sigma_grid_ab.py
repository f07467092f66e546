"""Time of the density query (crnerf_sigma_grid_* / crnerf_sigma_points_*, include/crnerf_geometry.h) against the route a caller had before it:
crnerf_posenc_f32 into [n,93] rows, then crnerf_mlp_forward_* with sigma_only.  One GPU, one run.

    python tools/sigma_grid_ab.py [--steps 10] [--warmup 3] [--chunk 4194304] [--no-resources] [--out FILE]

Bare ABI launches (ctypes on the loaded library, nothing else on the host side) on fixed buffers, INTERLEAVED G C P C' Q per round so that all
series see the same clocks: G the grid entry, P the points entry on the same points, C / C' the composed route -- launched twice per round, the
ratio of its two medians is its own run-to-run spread, the floor a new / composed ratio has to clear -- and Q the composed route's posenc
launches alone, the launch the new route does not have.  One pair of HIP events around every series member, the first `warmup` rounds discarded,
medians.  The composed route is handed the point list ready-made (a caller has to build it from the axes first: not charged) and runs in chunks of
`chunk` points, whose embedded rows (372 B a point) fit one buffer, as a caller must run it: a 256^3 grid is 6.2 GB of rows each way.
Workloads: 128^3 and 256^3 under both precisions, 512^3 under bf16.  Next to each ratio stands what the count predicts for the MLP kernel alone: the
trunk is 124 of 151 stages on the fp32 core, 992 of 1,208 fragments on the pair core (0.821 both).  A count, not a model of the clock.
Then, from the compile (hipcc -Rpass-analysis=kernel-resource-usage with build.py's flags): registers, scratch and occupancy of the new kernels
beside their stand-alone siblings."""
import argparse
import ctypes
import os
import re
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKLOADS = [("f32", 128), ("f32", 256), ("bf16", 128), ("bf16", 256), ("bf16", 512)]
COUNT = {"f32": 124 / 151.0, "bf16": 992 / 1208.0}
UNITS = {"sigma_query16.hip": ("sigma_points16_kernel", "sigma_grid16_kernel"), "mlp_forward16.hip": ("mlp_forward16_kernel",),
         "sigma_query_bf16p.hip": ("sigma_points_bf16p_kernel", "sigma_grid_bf16p_kernel"), "mlp_forward_bf16p.hip": ("mlp_forward_bf16p_kernel",)}


def timing(a, say):
    import torch
    sys.path.insert(0, ROOT)
    import crnerf_amd.synth as synth
    from crnerf_amd import _lib, ops
    dev = torch.device("cuda:0")
    lib = _lib.load()
    st = {k: torch.from_numpy(v).to(dev) for k, v in synth.mlp_state(21, 2.0).items()}
    vp = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    rows = torch.empty(a.chunk, 93, dtype=torch.float32, device=dev)        # the composed route's embedded rows, one chunk

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3

    say("rounds of G C P C' Q, %d timed after %d discarded, medians in us; composed route in chunks of %d points" % (a.steps, a.warmup, a.chunk))
    for precision, res in WORKLOADS:
        pk = ops.pack_mlp_weights(st, precision=precision)
        grid_fn, pts_fn = [getattr(lib, n) for n in ("crnerf_sigma_grid_" + precision, "crnerf_sigma_points_" + precision)]
        fwd_fn = getattr(lib, "crnerf_mlp_forward_" + precision)
        xs, ys, zs = (torch.linspace(lo, hi, res, device=dev) for lo, hi in ((-3.0, 3.0), (-2.0, 2.5), (-1.0, 4.0)))
        n = res ** 3
        Z, Y, X = torch.meshgrid(zs, ys, xs, indexing="ij")
        pts = torch.stack((X, Y, Z), dim=-1).reshape(-1, 3).contiguous()
        del X, Y, Z
        out_g, out_p, out_c = (torch.empty(n, dtype=torch.float32, device=dev) for _ in range(3))
        s = _lib.stream_ptr()
        chunks = [(i, min(a.chunk, n - i)) for i in range(0, n, a.chunk)]

        def grid():
            _lib.check(grid_fn(vp(pk), vp(xs), vp(ys), vp(zs), res, res, res, vp(out_g), s), "sigma_grid")

        def points():
            _lib.check(pts_fn(vp(pk), vp(pts), vp(out_p), n, s), "sigma_points")

        def composed():
            for i, m in chunks:
                _lib.check(lib.crnerf_posenc_f32(vp(pts[i:]), vp(rows), m, 15, s), "posenc")
                _lib.check(fwd_fn(vp(pk), vp(rows), vp(out_c[i:]), m, 1, s), "mlp_forward")

        def posenc_only():
            for i, m in chunks:
                _lib.check(lib.crnerf_posenc_f32(vp(pts[i:]), vp(rows), m, 15, s), "posenc")

        series = {k: [] for k in "GCPDQ"}
        for i in range(a.warmup + a.steps):
            t = (timed(grid), timed(composed), timed(points), timed(composed), timed(posenc_only))
            if i >= a.warmup:
                for k, v in zip("GCPDQ", t):
                    series[k].append(v)
        torch.cuda.synchronize()
        g, c, p, c2, q = (statistics.median(series[k]) for k in "GCPDQ")
        cm = 0.5 * (c + c2)
        same = "grid == points %s, == composed %s" % (torch.equal(out_g, out_p), torch.equal(out_g, out_c))
        if precision == "bf16":
            same += " (max |d| / (|sigma| + 1) %.2e)" % float(((out_g - out_c).abs() / (out_c.abs() + 1)).max())
        say("%-4s %3d^3 = %9d points, %2d chunk(s): grid %.1f (%.1f Mpt/s)  points %.1f (%.1f Mpt/s)  composed %.1f  composed' %.1f (C'/C %.4f; %.1f Mpt/s)"
            % (precision, res, n, len(chunks), g, n / g, p, n / p, c, c2, c2 / c, n / cm))
        say("       grid/composed %.4f  points/composed %.4f  count (MLP kernel alone) %.3f  |  posenc launches alone %.1f = %.3f of composed, "
            "(composed - posenc) %.1f: grid / that %.4f  |  %s" % (g / cm, p / cm, COUNT[precision], q, q / cm, cm - q, g / (cm - q), same))
        del pts, out_g, out_p, out_c


def resources(say):
    """VGPRs, scratch and occupancy of the new kernels and their stand-alone siblings, from the compiler's remarks (no GPU needed)."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("crnerf_build_for_sigma_ab", os.path.join(ROOT, "cr-nerf-pytorch_amd", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    say("")
    say("from the compile (-Rpass-analysis=kernel-resource-usage, build.py's flags per unit):")
    with tempfile.TemporaryDirectory() as tmp:
        procs = []
        for unit in UNITS:
            cmd = ([b._hipcc()] + [f for f in b.FLAGS if f != "-fPIC"] + b.PER_FILE_FLAGS.get(unit, []) +
                   ["-I", b.CSRC, "-S", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", os.path.join(b.CSRC, unit), "-o", os.path.join(tmp, unit + ".s")])
            procs.append((unit, subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)))
        for unit, p in procs:
            text = p.communicate()[0].decode(errors="replace")
            if p.returncode != 0:
                raise RuntimeError("hipcc failed on %s:\n%s" % (unit, text))
            for kernel in UNITS[unit]:
                m = re.search(r"Function Name: \S*%s\S*(.*?)(?=Function Name:|\Z)" % kernel, text, flags=re.S)
                get = lambda key: re.search(r"remark:\s+%s: (\d+)" % re.escape(key), m.group(1)).group(1)  # noqa: E731
                say("  %-22s %-28s VGPRs %s  AGPRs %s  SGPRs %s  scratch %s B/lane  occupancy %s waves/SIMD  LDS (static) %s B" % (
                    unit, kernel, get("VGPRs"), get("AGPRs"), get("TotalSGPRs"), get("ScratchSize [bytes/lane]"), get("Occupancy [waves/SIMD]"),
                    get("LDS Size [bytes/block]")))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--chunk", type=int, default=1 << 22)
    ap.add_argument("--no-resources", action="store_true")
    ap.add_argument("--no-timing", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
        if a.out:      # written as it grows: a run that is cut short leaves what it measured
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    say("tools/sigma_grid_ab.py   (one MI355X, one run)")
    say("The density query (include/crnerf_geometry.h; DESIGN 3.6 N10) against crnerf_posenc_f32 + crnerf_mlp_forward_*(sigma_only), the route a caller had.")
    if not a.no_timing:
        timing(a, say)
    if not a.no_resources:
        resources(say)


if __name__ == "__main__":
    main()

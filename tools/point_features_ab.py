"""Time and peak memory of the point-feature query (crnerf_feature_points_*, csrc/crnerf_point_features.h) against the route a caller had before it:
crnerf_posenc_f32 twice (points into [n,93] rows, directions into [n,27]), torch.cat into [n,120] rows, crnerf_mlp_forward_*, and the first 64 of
the 65 output columns.  One GPU, one run.

    python tools/point_features_ab.py [--steps 10] [--warmup 3] [--no-resources] [--no-timing] [--out FILE]

Bare ABI launches (ctypes on the loaded library; the composed route's cat is torch.cat(out=) into a fixed buffer) on fixed buffers, INTERLEAVED
N C N' C' per round so that all series see the same clocks: N / N' the new entry, C / C' the composed route -- each launched twice per round, the
ratio of the two medians is the route's own run-to-run spread, the floor a new / composed ratio has to clear.  One pair of HIP events around every
series member, the first `warmup` rounds discarded, medians.  The composed route's [n,65] output is left as it is: a caller who hands the features
to the decoder pays one more strided copy into [n,64] rows, which is not charged.
Workloads: the vertex counts of the trained meshes of profiles/r21/mesh.txt (128^3, 256^3, 512^3: 141 k, 778 k, 4.46 M) under both precisions; the
points are seeded uniforms in the density query's test ranges, the directions seeded unit vectors.
Peak memory: torch.cuda.max_memory_allocated over one untimed call of each route through crnerf_amd.ops (inputs resident, nothing else), minus what
was allocated before the call: what a caller sees.
Then, from the compile (hipcc -Rpass-analysis=kernel-resource-usage with build.py's flags): registers, scratch and occupancy of the new kernels
beside their siblings."""
import argparse
import ctypes
import os
import re
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [141206, 777812, 4457406]
UNITS = {"feature_query16.hip": ("feature_points16_kernel",), "mlp_forward16.hip": ("mlp_forward16_kernel",), "sigma_query16.hip": ("sigma_points16_kernel",),
         "feature_query_bf16p.hip": ("feature_points_bf16p_kernel",), "mlp_forward_bf16p.hip": ("mlp_forward_bf16p_kernel",),
         "sigma_query_bf16p.hip": ("sigma_points_bf16p_kernel",)}


def timing(a, say):
    import torch
    sys.path.insert(0, ROOT)
    import crnerf_amd.synth as synth
    from crnerf_amd import _lib, ops
    dev = torch.device("cuda:0")
    lib = _lib.load()
    st = {k: torch.from_numpy(v).to(dev) for k, v in synth.mlp_state(21, 2.0).items()}
    vp = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3

    def peak(fn):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        out = fn()
        torch.cuda.synchronize()
        top = torch.cuda.max_memory_allocated() - base
        del out
        return top

    say("rounds of N C N' C', %d timed after %d discarded, medians in us" % (a.steps, a.warmup))
    for precision in ("f32", "bf16"):
        pk = ops.pack_mlp_weights(st, precision=precision)
        new_fn = getattr(lib, "crnerf_feature_points_" + precision)
        fwd_fn = getattr(lib, "crnerf_mlp_forward_" + precision)
        for n in a.sizes:
            g = torch.Generator(device="cpu").manual_seed(n)
            pts = (torch.rand(n, 3, generator=g) * torch.tensor([6.0, 4.5, 5.0]) + torch.tensor([-3.0, -2.0, -1.0])).to(dev).contiguous()
            dirs = torch.nn.functional.normalize(torch.randn(n, 3, generator=g), dim=1).to(dev).contiguous()

            # peak memory first, through the Python layer, while nothing but the inputs is resident
            m_new = peak(lambda: ops.feature_points(pk, pts, dirs, precision=precision))
            m_comp = peak(lambda: ops.mlp_forward(pk, torch.cat((ops.posenc(pts, 15), ops.posenc(dirs, 4)), dim=1), precision=precision)[:, :64])

            feat, sig = torch.empty(n, 64, dtype=torch.float32, device=dev), torch.empty(n, dtype=torch.float32, device=dev)
            e_xyz, e_dir = torch.empty(n, 93, dtype=torch.float32, device=dev), torch.empty(n, 27, dtype=torch.float32, device=dev)
            rows, out = torch.empty(n, 120, dtype=torch.float32, device=dev), torch.empty(n, 65, dtype=torch.float32, device=dev)
            s = _lib.stream_ptr()

            def new():
                _lib.check(new_fn(vp(pk), vp(pts), vp(dirs), vp(feat), vp(sig), n, s), "feature_points")

            def composed():
                _lib.check(lib.crnerf_posenc_f32(vp(pts), vp(e_xyz), n, 15, s), "posenc")
                _lib.check(lib.crnerf_posenc_f32(vp(dirs), vp(e_dir), n, 4, s), "posenc")
                torch.cat((e_xyz, e_dir), dim=1, out=rows)
                _lib.check(fwd_fn(vp(pk), vp(rows), vp(out), n, 0, s), "mlp_forward")

            series = {k: [] for k in "NCMD"}
            for i in range(a.warmup + a.steps):
                t = (timed(new), timed(composed), timed(new), timed(composed))
                if i >= a.warmup:
                    for k, v in zip("NCMD", t):
                        series[k].append(v)
            torch.cuda.synchronize()
            t_n, t_c, t_n2, t_c2 = (statistics.median(series[k]) for k in "NCMD")
            nm, cm = 0.5 * (t_n + t_n2), 0.5 * (t_c + t_c2)
            same = "features == composed %s, sigma == composed %s" % (torch.equal(feat, out[:, :64]), torch.equal(sig, out[:, 64]))
            if precision == "bf16":
                same += " (max |d feature| %.2e, max |d sigma| / (|sigma| + 1) %.2e)" % (
                    float((feat - out[:, :64]).abs().max()), float(((sig - out[:, 64]).abs() / (out[:, 64].abs() + 1)).max()))
            say("%-4s n = %7d: new %.1f  new' %.1f (N'/N %.4f; %.2f Mpt/s)  composed %.1f  composed' %.1f (C'/C %.4f; %.2f Mpt/s)"
                % (precision, n, t_n, t_n2, t_n2 / t_n, n / nm, t_c, t_c2, t_c2 / t_c, n / cm))
            say("       new/composed %.4f  |  peak memory beyond the inputs: new %.1f MB (%.0f B/point)  composed %.1f MB (%.0f B/point)  new/composed %.4f  |  %s"
                % (nm / cm, m_new / 1e6, m_new / n, m_comp / 1e6, m_comp / n, m_new / m_comp, same))
            del pts, dirs, feat, sig, e_xyz, e_dir, rows, out


def resources(say):
    """VGPRs, scratch and occupancy of the new kernels and their siblings, from the compiler's remarks (no GPU needed)."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("crnerf_build_for_point_features_ab", os.path.join(ROOT, "cr-nerf-pytorch_amd", "build.py"))
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
                say("  %-24s %-28s VGPRs %s  AGPRs %s  SGPRs %s  SGPR spills %s  VGPR spills %s  scratch %s B/lane  occupancy %s waves/SIMD" % (
                    unit, kernel, get("VGPRs"), get("AGPRs"), get("TotalSGPRs"), get("SGPRs Spill"), get("VGPRs Spill"), get("ScratchSize [bytes/lane]"),
                    get("Occupancy [waves/SIMD]")))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sizes", type=int, nargs="+", default=SIZES)
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

    say("tools/point_features_ab.py   (one MI355X, one run)")
    say("The point-feature query (csrc/crnerf_point_features.h; DESIGN 3.6 N13) against crnerf_posenc_f32 x 2 + torch.cat + crnerf_mlp_forward_*, the route a caller had.")
    if not a.no_timing:
        timing(a, say)
    if not a.no_resources:
        resources(say)


if __name__ == "__main__":
    main()

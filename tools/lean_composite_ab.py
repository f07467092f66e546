"""Frame time of lean=True in the composite precisions "bf16_hc" and "bf16_fc" against the same call on the parent commit, one GPU.

    python tools/lean_composite_ab.py --parent-tree PATH [--frames 5] [--trace-dir DIR] [--lean-trace-dir DIR] [--fine-alone] [--out FILE]

What is timed: pipeline.render_frame(..., lean=True) at 800 x 800 (rays, render in 32,768-ray chunks, decode; the appearance embedding is handed
over), 64+128 and 256+256 samples, one pair of HIP events around every frame, the first frame of a series discarded, medians reported.
--parent-tree PATH: a checkout of the parent commit with its library built (on the parent the flag renders the composite modes as without it and
drops the other tensors).  Every series runs in a child process of its own that imports one tree; the children alternate P N P N, so the two P
series show the parent's run-to-run spread -- the noise floor an N / P ratio has to clear.  --child is that child's mode.
--trace-dir DIR: the output directory of

    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/lean_composite_ab.py --child --tree PARENT --no-lean --frames 2

(the parent's ordinary call).  From that one kernel trace the tool takes, per mode and sample count, the last frame's span (first kernel start to
last kernel end) and the time of its coarse launches (the h2 / fp16 coarse render and the x3 repair), and prints next to each measured ratio the
prediction 1 - 0.179 x coarse / frame: 0.179 is the share of the weight stream behind the trunk (432 of 2,416 fragments on the h2 core, 216 of
1,208 on the pair core).  A count, not a model of the clock: the part is power-governed, and the trunk tile's sigma head is no longer hidden.
--lean-trace-dir DIR: the same trace of this tree's lean call (--child --tree . --frames 2); the two traces' per-kernel times of a frame are
printed side by side: the coarse launch, the repair, the fine launch.
--fine-alone: the fine launch by itself, ops.render_rays_bf16_fine full against lean on fixed inputs, rounds of F L F' L in this process."""
import argparse
import csv
import glob
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = ("bf16_hc", "bf16_fc")
SAMPLES = ((64, 128), (256, 256))
COARSE_KERNELS = ("render_rays_h2_kernel", "render_rays_f16p_kernel", "render_coarse_weights", "render_rays_x3_kernel")
TAIL_SHARE = 0.179


def child(a):
    """One series per (mode, samples): `frames` timed frames after one discarded; prints one line each."""
    sys.path.insert(0, os.path.abspath(a.tree))
    import numpy as np
    import torch
    import crnerf_amd.synth as synth
    from crnerf_amd import pipeline
    dev = torch.device("cuda:0")
    st = [synth.mlp_state(s, 3.0, 1.0) for s in (1, 2)]
    focal = 800 / 2 / np.tan(np.pi / 6)
    K = np.array([[focal, 0, 400], [0, focal, 400], [0, 0, 1]])
    c2w = np.array([[1, 0, 0, 0.05], [0, -1, 0, 0.02], [0, 0, -1, 0.1]], dtype=np.float32)
    style = torch.rand(1, 64, 32, 32, device=dev, generator=torch.Generator(device=dev).manual_seed(0))
    with torch.no_grad():
        for nc, ni in SAMPLES:
            class HP:
                nerf_out_dim, pertubeCord, N_emb_xyz, N_emb_dir, use_disp, encode_a, encode_random, N_a = 64, False, 15, 4, False, True, True, 48
                img_wh, N_samples, N_importance = [800, 800], nc, ni
            hp = HP()
            m, emb = pipeline.get_model(hp, dev), pipeline.get_embeddings(hp)
            m["coarse"].load_state_dict({k: torch.from_numpy(v) for k, v in st[0].items()})
            m["fine"].load_state_dict({k: torch.from_numpy(v) for k, v in st[1].items()})
            m["decoder"].load_state_dict({k: torch.from_numpy(v) for k, v in synth.decoder_state(3).items()})
            for mode in MODES:
                ms, img = [], None
                for i in range(1 + a.frames):
                    torch.cuda.synchronize()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    img = pipeline.render_frame(m, emb, None, style, 800, 800, K, c2w, hp, chunk=32768, precision=mode, a_emb=style, lean=not a.no_lean)
                    e1.record()
                    torch.cuda.synchronize()
                    if i:
                        ms.append(e0.elapsed_time(e1))
                print("SERIES %s %d+%d median %.2f ms frames %s checksum %.6f" % (mode, nc, ni, statistics.median(ms), " ".join("%.2f" % v for v in ms),
                                                                                   float(img.double().sum())), flush=True)


def trace_shares(trace_dir):
    """{(mode, 'Nc+Ni'): (coarse ms, frame ms)} from the kernel trace of the child's ordinary call: series follow each other in the child's order, a
    frame starts at its ray-generation kernel, the last frame of every series is taken."""
    files = glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        return {}
    rows = []
    with open(files[0]) as f:
        for r in csv.DictReader(f):
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]))
    rows.sort()
    starts = [i for i, r in enumerate(rows) if "generate_rays" in r[2]]
    series = [(mode, "%d+%d" % s) for s in SAMPLES for mode in MODES]
    if not starts or len(starts) % len(series):
        return {}
    per = len(starts) // len(series)
    out = {}
    for k, key in enumerate(series):
        lo = starts[k * per + per - 1]
        hi = starts[k * per + per] if k * per + per < len(starts) else len(rows)
        frame = rows[lo:hi]
        coarse = sum(e - s for s, e, n in frame if any(c in n for c in COARSE_KERNELS))
        out[key] = (coarse / 1e6, (max(e for _, e, _ in frame) - frame[0][0]) / 1e6)
    return out


def frame_kernels(trace_dir):
    """{(mode, 'Nc+Ni'): {kernel name: ms}} of the last frame of every series of a child's kernel trace."""
    files = glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        return {}
    with open(files[0]) as f:
        rows = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]) for r in csv.DictReader(f))
    starts = [i for i, r in enumerate(rows) if "generate_rays" in r[2]]
    series = [(mode, "%d+%d" % s) for s in SAMPLES for mode in MODES]
    if not starts or len(starts) % len(series):
        return {}
    per, out = len(starts) // len(series), {}
    for k, key in enumerate(series):
        hi = starts[k * per + per] if k * per + per < len(starts) else len(rows)
        d = {}
        for s0, e0, n in rows[starts[k * per + per - 1]:hi]:
            n = n.split("(")[0].replace("crnerf::", "").replace("pcore_f16::", "")
            d[n] = d.get(n, 0.0) + (e0 - s0) / 1e6
        out[key] = d
    return out


def fine_alone(say):
    import torch
    sys.path.insert(0, ROOT)
    import crnerf_amd.synth as synth
    from crnerf_amd import ops
    dev = torch.device("cuda:0")
    st = [synth.mlp_state(s, 3.0, 1.0) for s in (1, 2)]
    pf = ops.pack_mlp_weights({k: torch.from_numpy(v).to(dev) for k, v in st[1].items()}, precision="bf16")
    px = ops.pack_mlp_weights({k: torch.from_numpy(v).to(dev) for k, v in st[0].items()}, precision="f32x3")

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3
    say("the fine launch alone, one process, rounds of F L F' L on fixed inputs (30 timed rounds after 8 discarded, events around every call):")
    with torch.no_grad():
        for nc, ni in SAMPLES:
            R = 32768
            rays = torch.from_numpy(synth.rays(R, seed=0)).to(dev)
            zs, u = torch.linspace(0, 1, nc, device=dev), torch.linspace(0, 1, ni, device=dev)
            wc = ops.render_coarse_weights(px, rays, nc, precision="f32x3", z_steps=zs)["weights_coarse"]
            full = lambda: ops.render_rays_bf16_fine(pf, rays, wc, nc, ni, z_steps=zs, u=u)  # noqa: E731
            lean = lambda: ops.render_rays_bf16_fine(pf, rays, wc, nc, ni, z_steps=zs, u=u, lean=True)  # noqa: E731
            t = {"F": [], "F'": [], "L": []}
            for i in range(8 + 30):
                for name, fn in (("F", full), ("L", lean), ("F'", full), ("L", lean)):
                    us = timed(fn)
                    if i >= 8:
                        t[name].append(us)
            m = statistics.median
            say("  fine launch %d x (%d+%d): full median %.1f us (F %.1f, F' %.1f), lean median %.1f us, lean/full %.4f, noise floor %.4f"
                % (R, nc, ni, m(t["F"] + t["F'"]), m(t["F"]), m(t["F'"]), m(t["L"]), m(t["L"]) / m(t["F"] + t["F'"]), abs(m(t["F"]) / m(t["F'"]) - 1)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=5)
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--trace-dir", default=None)
    ap.add_argument("--lean-trace-dir", default=None)
    ap.add_argument("--fine-alone", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--tree", default=ROOT)
    ap.add_argument("--no-lean", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a)
    lines = []

    def say(s):
        lines.append(s)
        print(s, flush=True)
    say("800 x 800 pipeline.render_frame(lean=True), 32,768-ray chunks; %d timed frames per series after one discarded; child processes alternate "
        "between the parent commit (P) and this tree (N)" % a.frames)
    got = {}
    for tag, tree in (("P", a.parent_tree), ("N", ROOT), ("P", a.parent_tree), ("N", ROOT)):
        if tree is None:
            continue
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--tree", tree, "--frames", str(a.frames)],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
        if r.returncode != 0:
            say("  child failed (%d): %s" % (r.returncode, r.stdout[-600:]))
            break
        for ln in r.stdout.splitlines():
            if ln.startswith("SERIES "):
                f = ln.split()
                got.setdefault((f[1], f[2]), {}).setdefault(tag, []).append((float(f[4]), f[-1]))
                say("  %s %s" % (tag, ln[7:]))
    shares = trace_shares(a.trace_dir) if a.trace_dir else {}
    for key, t in got.items():
        if "P" not in t or "N" not in t:
            continue
        p, n = [v for v, _ in t["P"]], [v for v, _ in t["N"]]
        spread = (max(p) - min(p)) / statistics.mean(p)
        line = "%s %s: parent %.2f ms (series %s; spread %.4f), lean %.2f ms (series %s), lean/parent %.3f; same image: %s" % (
            key[0], key[1], statistics.mean(p), " ".join("%.2f" % v for v in p), spread, statistics.mean(n), " ".join("%.2f" % v for v in n),
            statistics.mean(n) / statistics.mean(p), len({c for _, c in t["P"] + t["N"]}) == 1)
        if key in shares:
            c, fr = shares[key]
            line += "; parent's trace: coarse launches %.2f ms of a %.2f ms frame, predicted %.3f" % (c, fr, 1.0 - TAIL_SHARE * c / fr)
        say(line)
    if a.trace_dir and a.lean_trace_dir:
        P, N = frame_kernels(a.trace_dir), frame_kernels(a.lean_trace_dir)
        say("kernel time per 800 x 800 frame (20 launches each), one rocprofv3 kernel trace per side: the parent's ordinary call -> this tree's lean call")
        for key in P:
            if key not in N:
                continue
            p, n = P[key], N[key]
            pc = "render_rays_h2_kernel" if key[0] == "bf16_hc" else "render_rays_f16p_kernel"
            nc = "render_coarse_weights_h2_kernel" if key[0] == "bf16_hc" else "render_coarse_weights_f16p_kernel"
            pf, nf = "render_rays_bf16p_fine_kernel", "render_rays_bf16p_lean_fine_kernel"
            if not all(k in d for d, ks in ((p, (pc, pf, "render_rays_x3_kernel")), (n, (nc, nf, "render_coarse_weights_x3_kernel"))) for k in ks):
                continue
            say("%s %s: coarse %s %.2f ms -> %s %.2f ms (%.3f); repair %.2f -> %.2f ms; fine %s %.2f ms -> %s %.2f ms (%.3f); all kernels %.2f -> %.2f ms"
                % (key[0], key[1], pc, p[pc], nc, n[nc], n[nc] / p[pc], p["render_rays_x3_kernel"], n["render_coarse_weights_x3_kernel"], pf, p[pf], nf, n[nf],
                   n[nf] / p[pf], sum(p.values()), sum(n.values())))
    if a.fine_alone:
        fine_alone(say)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

"""Host time of the render entry layer (csrc/abi.hip render_entry, ops._render) against the parent commit, one GPU.  Nothing on the device differs
between the two, so what can move is host time per call.

    python tools/render_entries_ab.py --parent-tree PATH [--reps 5] [--bench-steps 20] [--out FILE]

--parent-tree PATH: a checkout of the parent commit with its library built, bench.py and oracle/ beside the package.  Three measurements, each in
child processes that import one tree and alternate P N P N ... (--reps of each):
  (i)   calls: wall time of 2,000 back-to-back ops.render_rays(..., train=True, precision="f32") at R = 1,024, 64 + 64 samples, one synchronise at
        the end (200 discarded calls in front).  Alone, this call is device-bound (1.85 ms of kernel per call, and the queue fills: the time to
        enqueue is the device's too), so it bounds the host time per call without isolating it; (iii) has the figure that does;
  (ii)  frame: one 800 x 800 pipeline.render_frame under "bf16_hc" with lean=True, HIP events around it (one discarded frame in front);
  (iii) bench: bench.py --gpus 1 as it is, the "value" of its JSON line (rays/s), and beside it
        host: that line's timing.host_enqueue_ms median -- the host time to enqueue one step (render_rays_cross_ray + the decoder).
Per measurement: every repetition, the medians, and the parent's own spread across its repetitions (max - min), which is what this tree's median may
exceed the parent's by."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS, R, NC, NI = 2000, 1024, 64, 64


def child(tree):
    sys.path.insert(0, os.path.abspath(tree))
    import numpy as np
    import torch
    import crnerf_amd.synth as synth
    from crnerf_amd import ops, pipeline
    dev = torch.device("cuda:0")
    st = [synth.mlp_state(s, 3.0, 1.0) for s in (1, 2)]
    pc, pf = (ops.pack_mlp_weights({k: torch.from_numpy(v).to(dev) for k, v in s.items()}) for s in st)
    rays = torch.from_numpy(synth.rays(R, seed=0, H=32, W=32)).to(dev)
    zt, ut = torch.linspace(0, 1, NC, device=dev), torch.linspace(0, 1, NI, device=dev)
    with torch.no_grad():
        for n in (200, CALLS):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(n):
                ops.render_rays(pc, pf, rays, NC, NI, z_steps=zt, u=ut, train=True, precision="f32")
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
        print("CALLS %.3f" % (dt * 1e3), flush=True)

        class HP:
            nerf_out_dim, pertubeCord, N_emb_xyz, N_emb_dir, use_disp, encode_a, encode_random, N_a = 64, False, 15, 4, False, True, True, 48
            img_wh, N_samples, N_importance = [800, 800], 64, 128
        hp = HP()
        m, emb = pipeline.get_model(hp, dev), pipeline.get_embeddings(hp)
        m["coarse"].load_state_dict({k: torch.from_numpy(v) for k, v in st[0].items()})
        m["fine"].load_state_dict({k: torch.from_numpy(v) for k, v in st[1].items()})
        m["decoder"].load_state_dict({k: torch.from_numpy(v) for k, v in synth.decoder_state(3).items()})
        focal = 800 / 2 / np.tan(np.pi / 6)
        K = np.array([[focal, 0, 400], [0, focal, 400], [0, 0, 1]])
        c2w = np.array([[1, 0, 0, 0.05], [0, -1, 0, 0.02], [0, 0, -1, 0.1]], dtype=np.float32)
        style = torch.rand(1, 64, 32, 32, device=dev, generator=torch.Generator(device=dev).manual_seed(0))
        for i in range(2):
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            img = pipeline.render_frame(m, emb, None, style, 800, 800, K, c2w, hp, chunk=32768, precision="bf16_hc", a_emb=style, lean=True)
            e1.record()
            torch.cuda.synchronize()
        print("FRAME %.3f checksum %.6f" % (e0.elapsed_time(e1), float(img.double().sum())), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-tree")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--bench-steps", type=int, default=20)
    ap.add_argument("--out")
    ap.add_argument("--child")
    a = ap.parse_args()
    if a.child:
        return child(a.child)
    trees = {"P": os.path.abspath(a.parent_tree), "N": ROOT}
    got = {k: {"calls": [], "host": [], "frame": [], "bench": []} for k in trees}
    lines = ["render entry layer, parent commit (P) against this tree (N): child processes alternating P N, %d of each" % a.reps]

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def run(cmd):
        return subprocess.run(cmd, check=True, stdout=subprocess.PIPE, text=True, timeout=300).stdout

    for rep in range(a.reps):
        for k, tree in trees.items():
            out = run([sys.executable, os.path.abspath(__file__), "--child", tree])
            calls = float([ln for ln in out.splitlines() if ln.startswith("CALLS")][0].split()[1])
            frame = [ln for ln in out.splitlines() if ln.startswith("FRAME")][0].split()
            got[k]["calls"].append(calls)
            got[k]["frame"].append(float(frame[1]))
            say("  %s rep %d: %d train calls %.1f ms (%.2f us per call); frame %.2f ms, checksum %s" % (k, rep, CALLS, calls, calls * 1e3 / CALLS, float(frame[1]), frame[3]))
    for rep in range(a.reps):
        for k, tree in trees.items():
            out = run([sys.executable, os.path.join(tree, "bench.py"), "--gpus", "1", "--steps", str(a.bench_steps), "--warmup", "5"])
            line = [json.loads(ln) for ln in out.splitlines() if ln.startswith("{") and '"metric"' in ln][-1]
            got[k]["bench"].append(1e6 / line["value"])
            got[k]["host"].append(1e3 * line["timing"]["host_enqueue_ms"]["median"])
            say("  %s rep %d: bench.py %.0f %s (%.4f us per ray), host enqueue %.1f us per step" % (k, rep, line["value"], line["unit"], 1e6 / line["value"], got[k]["host"][-1]))
    for what, unit in (("calls", "ms per %d calls" % CALLS), ("frame", "ms per frame"), ("bench", "us per ray"),
                       ("host", "us of host enqueue per bench.py step")):
        p, n = got["P"][what], got["N"][what]
        spread, d = max(p) - min(p), statistics.median(n) - statistics.median(p)
        say("%s (%s): parent median %.4f (min %.4f, max %.4f, spread %.4f), this tree median %.4f (min %.4f, max %.4f); this tree - parent = %+.4f: %s"
            % (what, unit, statistics.median(p), min(p), max(p), spread, statistics.median(n), min(n), max(n), d,
               "within the parent's spread" if d <= spread else "BEYOND the parent's spread"))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

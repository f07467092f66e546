"""Time of the lean render on the fp32-accurate split cores (crnerf_render_rays_lean_f32x3 / _f32h2, include/crnerf_lean_x.h) against the full one, one GPU.

    python tools/lean_x_ab.py [--steps 30] [--warmup 8] [--parent-tree PATH] [--frames 5] [--out FILE]

Kernel: bare ABI launches on fixed buffers (launcher=True: nothing but the C call on the host side), INTERLEAVED F L F' L so that all series see the
same clocks; one pair of HIP events around every launch, the first `warmup` rounds discarded; medians.  The full kernel is launched twice per round
(F and F'): the ratio of those two medians is the full kernel's own run-to-run spread, the noise floor a lean / full ratio has to clear.
Workloads: "f32h2" and "f32x3" at 1,024 x (64+128) and 4,096 x (256+256).  Next to each ratio stands what the MFMA / weight-stream count predicts:
a coarse tile walks 1,984 of 2,416 fragments on h2 (0.821) and 2,976 of 3,648 on x3 (0.816), so with 32-sample tiles the lean kernel walks
(t Tc + Tf) / (Tc + Tf) of the full kernel's stream, Tc = ceil(Nc / 32), Tf = ceil((Nc + Ni) / 32).  A count, not a model of the clock.
--parent-tree PATH: a checkout of the parent commit with its library built.  Frame: one 800 x 800 pipeline.render_frame(precision="auto",
lean=True) at 64+128 and 256+256 (rays, render in 32,768-ray chunks, decode), one pair of HIP events per frame, the first frame discarded, medians;
every series in a child process that imports one tree, alternating P N P N -- on the parent the flag renders in full and drops the other tensors,
and the two P series show the run-to-run spread.  The image checksum (float64 sum) and its SHA-1 are printed per series: the trees must agree.
--child is that child's mode."""
import argparse
import hashlib
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKLOADS = [(1024, 64, 128), (4096, 256, 256)]
SAMPLES = ((64, 128), (256, 256))
TRUNK_SHARE = {"f32h2": 1984 / 2416.0, "f32x3": 2976 / 3648.0}


def predicted(precision, nc, ni):
    tc, tf = (nc + 31) // 32, (nc + ni + 31) // 32
    return (TRUNK_SHARE[precision] * tc + tf) / float(tc + tf)


def kernel_ab(a, say):
    import torch
    sys.path.insert(0, ROOT)
    import crnerf_amd.synth as synth
    from crnerf_amd import ops
    dev = torch.device("cuda:0")
    st = [{k: torch.from_numpy(v).to(dev) for k, v in synth.mlp_state(s, 3.0, 1.0).items()} for s in (1, 2)]
    auto = [ops.pack_mlp_weights(s, precision="auto") for s in st]

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3

    say("kernel: rounds of F L F' L, %d timed after %d discarded, medians in us" % (a.steps, a.warmup))
    with torch.no_grad():
        for precision in ("f32h2", "f32x3"):
            pc, pf = [(p.h2 if precision == "f32h2" else p.x3) for p in auto]
            for R, nc, ni in WORKLOADS:
                rays = torch.from_numpy(synth.rays(R, seed=0)).to(dev)
                kw = dict(z_steps=torch.linspace(0, 1, nc, device=dev), u=torch.linspace(0, 1, ni, device=dev))
                full, fo = ops.render_rays(pc, pf, rays, nc, ni, precision=precision, launcher=True, **kw)
                lean, lo = ops.render_rays_lean_x(pc, pf, rays, nc, ni, precision=precision, launcher=True, **kw)
                f, f2, l = [], [], []
                for i in range(a.warmup + a.steps):
                    t = (timed(full), timed(lean), timed(full), timed(lean))
                    if i >= a.warmup:
                        f.append(t[0]); l.append(t[1]); f2.append(t[2]); l.append(t[3])
                torch.cuda.synchronize()
                same = all(torch.equal(lo[k], fo[k]) for k in ("feature_fine", "depth_fine"))
                mf, mf2, ml = statistics.median(f), statistics.median(f2), statistics.median(l)
                say("%s %5d x (%d+%d): full %.1f  full' %.1f (F'/F %.4f)  lean %.1f  lean/full %.4f  count %.3f  bit-identical %s" % (
                    precision, R, nc, ni, mf, mf2, mf2 / mf, ml, ml / (0.5 * (mf + mf2)), predicted(precision, nc, ni), same))


def child(a):
    """One series per sample count: `frames` timed frames after one discarded; prints one line each."""
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
            ms, img = [], None
            for i in range(1 + a.frames):
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                img = pipeline.render_frame(m, emb, None, style, 800, 800, K, c2w, hp, chunk=32768, precision="auto", a_emb=style, lean=True)
                e1.record()
                torch.cuda.synchronize()
                if i:
                    ms.append(e0.elapsed_time(e1))
            sha = hashlib.sha1(img.contiguous().cpu().numpy().tobytes()).hexdigest()[:16]
            print("SERIES auto %d+%d median %.2f ms frames %s checksum %.6f sha1 %s" % (nc, ni, statistics.median(ms), " ".join("%.2f" % v for v in ms),
                                                                                       float(img.double().sum()), sha), flush=True)


def frame_ab(a, say):
    say("frame: 800 x 800 render_frame(precision='auto', lean=True), children P N P N, %d frames each after one discarded" % a.frames)
    series = {}
    for tag, tree in (("P", a.parent_tree), ("N", ROOT), ("P", a.parent_tree), ("N", ROOT)):
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--tree", tree, "--frames", str(a.frames)], stdout=subprocess.PIPE,
                             stderr=subprocess.STDOUT, timeout=600)
        if out.returncode != 0:
            say("child %s failed (rc %d):\n%s" % (tag, out.returncode, out.stdout.decode(errors="replace")[-2000:]))
            return 1
        for line in out.stdout.decode().splitlines():
            if line.startswith("SERIES"):
                w = line.split()
                say("%s %s" % (tag, line))
                series.setdefault(w[2], []).append((tag, float(w[4]), w[-1]))
    for key, rows in series.items():
        p, n = [r[1] for r in rows if r[0] == "P"], [r[1] for r in rows if r[0] == "N"]
        say("auto %s: parent %s ms (P'/P %.4f)  this tree %s ms  N/P %.4f  image bit-identical %s" % (
            key, " ".join("%.2f" % v for v in p), p[1] / p[0], " ".join("%.2f" % v for v in n), statistics.mean(n) / statistics.mean(p),
            len({r[2] for r in rows}) == 1))
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--frames", type=int, default=5)
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--tree", default=ROOT)
    ap.add_argument("--no-kernel", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.child:
        return child(a)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    rc = 0
    if not a.no_kernel:
        kernel_ab(a, say)
    if a.parent_tree:
        rc = frame_ab(a, say)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return rc


if __name__ == "__main__":
    sys.exit(main())

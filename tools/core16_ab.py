"""One leg of an A/B of the fp32 render core (csrc/mlp_core16.h): kernel time of crnerf_render_rays_f32 in THIS process' library.

    CRNERF_LIB_PATH=cr-nerf-pytorch_amd/variants/libcrnerf_NAME.so python tools/core16_ab.py [--steps 200] [--warmup 20] [--tag NAME] [--out FILE]

Bare ABI launches of the headline batch, 1,024 rays x (64+128), on fixed buffers (ops.render_rays(..., launcher=True): nothing but the C call on
the host side), one pair of HIP events around every launch, the first `warmup` discarded.  Prints, and appends to --out, one line: tag, median,
min, max in microseconds and a SHA-256 over every output of the last launch (two builds that compute the same thing print the same digest).
The part is power-governed, so builds are compared by alternating processes -- P V P V ..., at least three of each -- never by one long run each;
a variant counts when each of its runs beats the parent's fastest and its median gain is at least twice the parent's own min-to-max spread
(of the per-process medians).

    python tools/core16_ab.py --judge FILE [--parent-tag parent]

reads the lines an --out file collected (no GPU needed) and applies that rule to every other tag."""
import argparse
import hashlib
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def judge(path, parent_tag):
    med = {}
    for line in open(path):
        f = line.split()
        if len(f) > 3 and f[1] == "median":
            med.setdefault(f[0], []).append(float(f[2]))
    par = med.pop(parent_tag)
    pm, spread = statistics.median(par), max(par) - min(par)
    print("%s: %d processes, medians %.1f .. %.1f us, median of medians %.1f, min-to-max spread %.1f us (%.2f %%); bar for a lever: every run below "
          "%.1f and a gain of at least %.1f us" % (parent_tag, len(par), min(par), max(par), pm, spread, 100 * spread / pm, min(par), 2 * spread))
    for tag, v in med.items():
        gain = pm - statistics.median(v)
        below = max(v) < min(par)
        print("%-9s medians %s -> median %.1f us, %.1f us (%.2f %%) %s than the parent, every run below the parent's fastest: %s -> %s" % (
            tag, ", ".join("%.1f" % x for x in v), statistics.median(v), abs(gain), 100 * abs(gain) / pm, "faster" if gain > 0 else "slower", below,
            "ACCEPTED" if below and gain >= 2 * spread else "did not pay"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--judge", metavar="FILE", default=None)
    ap.add_argument("--parent-tag", default="parent")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--tag", default=os.path.basename(os.environ.get("CRNERF_LIB_PATH", "shipped")))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.judge:
        return judge(a.judge, a.parent_tag)
    import torch
    import crnerf_amd.synth as synth
    from crnerf_amd import ops

    dev = torch.device("cuda:0")
    st = [{k: torch.from_numpy(v).to(dev) for k, v in synth.mlp_state(s, 3.0, 1.0).items()} for s in (1, 2)]
    pc, pf = ops.pack_mlp_weights(st[0]), ops.pack_mlp_weights(st[1])
    R, nc, ni = 1024, 64, 128
    rays = torch.from_numpy(synth.rays(R, seed=0)).to(dev)
    with torch.no_grad():
        launch, out = ops.render_rays(pc, pf, rays, nc, ni, z_steps=torch.linspace(0, 1, nc, device=dev), u=torch.linspace(0, 1, ni, device=dev),
                                      want_z_fine=True, launcher=True)
        times = []
        for i in range(a.warmup + a.steps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            launch()
            e1.record()
            e1.synchronize()
            if i >= a.warmup:
                times.append(e0.elapsed_time(e1) * 1e3)
    h = hashlib.sha256()
    for k in sorted(out):
        h.update(out[k].cpu().numpy().tobytes())
    line = "%-28s median %8.1f us  min %8.1f  max %8.1f  (%d launches)  outputs sha256 %s" % (
        a.tag, statistics.median(times), min(times), max(times), len(times), h.hexdigest()[:16])
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

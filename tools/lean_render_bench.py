"""Kernel time of the lean inference render (crnerf_render_rays_lean_f32) against the full one (crnerf_render_rays_f32), one GPU, one process.

    python tools/lean_render_bench.py [--steps 40] [--warmup 10] [--frame] [--out FILE]

Bare ABI launches on fixed buffers (ops.render_rays(..., launcher=True): nothing but the C call on the host side), full and lean INTERLEAVED
(F L F L ...) so that both see the same clocks, one pair of HIP events around every launch, the first `warmup` pairs discarded; medians reported.
Workloads: 1,024 x (64+128), the headline batch, and 4,096 x (256+256), the reference's eval recipe.  Next to the measured lean / full ratio the
tool prints what the weight stream's arithmetic predicts: a coarse tile walks 124 of its 151 stages, so the kernel does
1 - (27/151) * coarse_steps / (coarse_steps + fine_steps) of the full kernel's MFMAs -- 0.955 and 0.940.  The part is power-governed: the clock may
give back, or add to, that saving.
--frame: additionally one 800 x 800 frame of pipeline.batched_inference at 256+256 in 32,768-ray chunks, full against lean, each with its
torch.cuda.max_memory_allocated."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WORKLOADS = [(1024, 64, 128), (4096, 256, 256)]


def predicted(nc, ni):
    sc, sf = (nc + 31) // 32, (nc + ni + 31) // 32
    return 1.0 - (27.0 / 151.0) * sc / (sc + sf)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--frame", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import crnerf_amd.synth as synth
    from crnerf_amd import ops

    dev = torch.device("cuda:0")
    lines = ["device: %s; %d timed pairs after %d discarded, full and lean interleaved, events around every launch" % (
        torch.cuda.get_device_name(0), a.steps, a.warmup)]
    say = lambda s: (lines.append(s), print(s, flush=True))  # noqa: E731
    print(lines[0], flush=True)
    st = [{k: torch.from_numpy(v).to(dev) for k, v in synth.mlp_state(s, 3.0, 1.0).items()} for s in (1, 2)]
    pc, pf = ops.pack_mlp_weights(st[0]), ops.pack_mlp_weights(st[1])
    with torch.no_grad():
        for R, nc, ni in WORKLOADS:
            rays = torch.from_numpy(synth.rays(R, seed=0)).to(dev)
            kw = dict(z_steps=torch.linspace(0, 1, nc, device=dev), u=torch.linspace(0, 1, ni, device=dev), launcher=True)
            full, out_f = ops.render_rays(pc, pf, rays, nc, ni, **kw)
            lean, out_l = ops.render_rays(pc, pf, rays, nc, ni, lean=True, **kw)
            times = {"full": [], "lean": []}
            for i in range(a.warmup + a.steps):
                for name, fn in (("full", full), ("lean", lean)):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    fn()
                    e1.record()
                    e1.synchronize()
                    if i >= a.warmup:
                        times[name].append(e0.elapsed_time(e1) * 1e3)
            same = torch.equal(out_f["feature_fine"], out_l["feature_fine"]) and torch.equal(out_f["depth_fine"], out_l["depth_fine"])
            mf, ml = statistics.median(times["full"]), statistics.median(times["lean"])
            say("%5d x (%d+%d): full median %.1f us (min %.1f, max %.1f)  lean median %.1f us (min %.1f, max %.1f)  lean/full %.3f  "
                "predicted by the stream %.3f  outputs bit-identical: %s" % (R, nc, ni, mf, min(times["full"]), max(times["full"]), ml, min(times["lean"]),
                                                                           max(times["lean"]), ml / mf, predicted(nc, ni), same))
        if a.frame:
            from crnerf_amd import pipeline

            class HP:
                nerf_out_dim, pertubeCord, N_emb_xyz, N_emb_dir, use_disp, encode_a, encode_random, N_a = 64, False, 15, 4, False, True, True, 48
                img_wh, N_samples, N_importance = [800, 800], 256, 256
            hp = HP()
            m, emb = pipeline.get_model(hp, dev), pipeline.get_embeddings(hp)
            m["coarse"].load_state_dict({k: torch.from_numpy(v) for k, v in synth.mlp_state(1, 3.0, 1.0).items()})
            m["fine"].load_state_dict({k: torch.from_numpy(v) for k, v in synth.mlp_state(2, 3.0, 1.0).items()})
            rays = torch.from_numpy(synth.rays(800 * 800, seed=0, H=800, W=800)).to(dev)
            del full, lean, out_f, out_l
            for name, flag in (("full", False), ("lean", True)):
                torch.cuda.synchronize()
                torch.cuda.empty_cache()
                torch.cuda.reset_peak_memory_stats()
                base = torch.cuda.memory_allocated()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                res = pipeline.batched_inference(m, emb, rays, None, 256, 256, False, 32768, False, args=hp, lean=flag)
                e1.record()
                torch.cuda.synchronize()
                peak = torch.cuda.max_memory_allocated() - base
                kept = sum(v.numel() * v.element_size() for k, v in res.items() if k != "feature_fine_random")
                say("800 x 800 batched_inference at 256+256, %s: peak memory above the inputs %.3f GB, returned tensors %.3f GB, %.0f ms (a single run)"
                    "" % (name, peak / 1e9, kept / 1e9, e0.elapsed_time(e1)))
                del res
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

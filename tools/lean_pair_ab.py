"""Kernel time of the lean inference render on the pair core (crnerf_render_rays_lean_bf16 / _f16) against the full one (crnerf_render_rays_bf16 /
_f16), one GPU.

    python tools/lean_pair_ab.py [--steps 40] [--warmup 10] [--frame] [--out FILE]

Bare ABI launches on fixed buffers (ops.render_rays(..., launcher=True): nothing but the C call on the host side), INTERLEAVED F L F' L F L ... so
that all series see the same clocks; one pair of HIP events around every launch, the first `warmup` rounds discarded; medians reported.  The full
kernel is launched twice per round (F and F'): the ratio of the two series' medians is the full kernel's own run-to-run spread, the noise floor a
lean / full ratio has to clear.  Workloads: 1,024 x (64+128), the headline batch, and 4,096 x (256+256), the reference's eval recipe.
Next to the measured ratio the tool prints what the MFMA count predicts: a pass is walked in 64-sample steps, one 32-point tile per wave and step,
and a coarse tile's trunk is 992 of its 1,208 fragments, so the lean kernel issues (992 Sc + 1208 Sf) / (1208 (Sc + Sf)) of the full kernel's MFMAs
with Sc = ceil(Nc / 64) and Sf = ceil((Nc + Ni) / 64): 0.928 and 0.940.  A count, not a model of the clock: the part is power-governed.
--frame: additionally one 800 x 800 pipeline.render_frame at 256+256, precision "bf16", in 32,768-ray chunks, full against lean, interleaved; each
with its torch.cuda.max_memory_allocated (reported, not promised: the Python layer drops the per-chunk tensors either way)."""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WORKLOADS = [(1024, 64, 128), (4096, 256, 256)]
TRUNK, WALK = 992, 1208


def predicted(nc, ni):
    sc, sf = (nc + 63) // 64, (nc + ni + 63) // 64
    return (TRUNK * sc + WALK * sf) / float(WALK * (sc + sf))


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3


def med(v):
    return statistics.median(v)


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
    lines = []

    def say(s):
        lines.append(s)
        print(s, flush=True)
    say("device: %s; %d timed rounds after %d discarded; a round is F L F' L (full, lean, full again, lean), events around every launch"
        % (torch.cuda.get_device_name(0), a.steps, a.warmup))
    st = [synth.mlp_state(s, 3.0, 1.0) for s in (1, 2)]
    with torch.no_grad():
        for prec in ("bf16", "f16"):
            pc, pf = (ops.pack_mlp_weights({k: torch.from_numpy(v).to(dev) for k, v in s.items()}, precision=prec) for s in st)
            for R, nc, ni in WORKLOADS:
                rays = torch.from_numpy(synth.rays(R, seed=0)).to(dev)
                kw = dict(z_steps=torch.linspace(0, 1, nc, device=dev), u=torch.linspace(0, 1, ni, device=dev), launcher=True, precision=prec)
                full, out_f = ops.render_rays(pc, pf, rays, nc, ni, **kw)
                lean, out_l = ops.render_rays(pc, pf, rays, nc, ni, lean=True, **kw)
                t = {"F": [], "F'": [], "L": []}
                for i in range(a.warmup + a.steps):
                    for name, fn in (("F", full), ("L", lean), ("F'", full), ("L", lean)):
                        us = timed(fn)
                        if i >= a.warmup:
                            t[name].append(us)
                same = torch.equal(out_f["feature_fine"], out_l["feature_fine"]) and torch.equal(out_f["depth_fine"], out_l["depth_fine"])
                mf, ml = med(t["F"] + t["F'"]), med(t["L"])
                floor = abs(med(t["F"]) / med(t["F'"]) - 1.0)
                q = np.percentile(t["F"] + t["F'"], [25, 75])
                say("%s %5d x (%d+%d): full median %.1f us (F %.1f, F' %.1f; quartiles %.1f .. %.1f)  lean median %.1f us (min %.1f, max %.1f)  "
                    "lean/full %.3f  predicted by the MFMA count %.3f  noise floor (F vs F') %.4f, interquartile / median %.4f  outputs bit-identical: %s"
                    % (prec, R, nc, ni, mf, med(t["F"]), med(t["F'"]), q[0], q[1], ml, min(t["L"]), max(t["L"]), ml / mf, predicted(nc, ni), floor,
                       (q[1] - q[0]) / mf, same))
                del lean, out_l
            del full, out_f
        if a.frame:
            from crnerf_amd import pipeline

            class HP:
                nerf_out_dim, pertubeCord, N_emb_xyz, N_emb_dir, use_disp, encode_a, encode_random, N_a = 64, False, 15, 4, False, True, True, 48
                img_wh, N_samples, N_importance = [800, 800], 256, 256
            hp = HP()
            m, emb = pipeline.get_model(hp, dev), pipeline.get_embeddings(hp)
            m["coarse"].load_state_dict({k: torch.from_numpy(v) for k, v in st[0].items()})
            m["fine"].load_state_dict({k: torch.from_numpy(v) for k, v in st[1].items()})
            m["decoder"].load_state_dict({k: torch.from_numpy(v) for k, v in synth.decoder_state(3).items()})
            enc = pipeline.encoder_sameoutputsize(64).to(dev)
            enc.load_state_dict({k: torch.from_numpy(v) for k, v in synth.encoder_state(4, 2.0).items()})
            focal = 800 / 2 / np.tan(np.pi / 6)
            K = np.array([[focal, 0, 400], [0, focal, 400], [0, 0, 1]])
            c2w = np.array([[1, 0, 0, 0.05], [0, -1, 0, 0.02], [0, 0, -1, 0.1]], dtype=np.float32)
            photo = torch.rand(1, 3, 100, 100, device=dev, generator=torch.Generator(device=dev).manual_seed(0))
            frame = lambda flag: pipeline.render_frame(m, emb, enc, photo, 800, 800, K, c2w, hp, chunk=32768, precision="bf16", lean=flag)  # noqa: E731
            imgs, ms, peak = {}, {False: [], True: []}, {}
            for i in range(1 + 3):                       # one discarded round, three timed ones, full and lean alternating
                for flag in (False, True):
                    torch.cuda.synchronize()
                    torch.cuda.empty_cache()
                    torch.cuda.reset_peak_memory_stats()
                    base = torch.cuda.memory_allocated()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    imgs[flag] = frame(flag)
                    e1.record()
                    torch.cuda.synchronize()
                    peak[flag] = torch.cuda.max_memory_allocated() - base
                    if i:
                        ms[flag].append(e0.elapsed_time(e1))
            say("800 x 800 render_frame at 256+256, precision bf16 (encoder + rays + render + decode), three frames each, alternating: full %s ms, "
                "lean %s ms; medians %.1f / %.1f, lean/full %.3f; peak memory above the models full %.3f GB, lean %.3f GB; same image: %s"
                % (["%.1f" % v for v in ms[False]], ["%.1f" % v for v in ms[True]], med(ms[False]), med(ms[True]), med(ms[True]) / med(ms[False]),
                   peak[False] / 1e9, peak[True] / 1e9, torch.equal(imgs[False], imgs[True])))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

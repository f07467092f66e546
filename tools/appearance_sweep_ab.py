"""The appearance sweep against what it replaces, one GPU.

    python tools/appearance_sweep_ab.py [--part a|b|ab|trace] [--steps 20] [--warmup 5] [--frames 8] [--out FILE]

Part (a), decode only, 800 x 800 and 320 x 240 content grids, S in {1, 4, 8, 16} styles of 32 x 32: ops.crossray_decode_multi (M; float planes, and
U = the uint8 frames) against S calls of ops.crossray_decode (N), INTERLEAVED M N U M N U ... so that all series see the same clocks; one pair of
HIP events around every series' work, the first `warmup` rounds discarded, medians reported.  N is what a caller with S photos runs today; it also
redoes the style statistics S times per frame, which the sweep does once (ops.crossray_style_stats, timed apart).  Next to the measured ratio the
tool prints what the byte counts of the apply pass predict, (256 + 12 S) / (268 S): a count of one stage, not a model of the whole decode -- the
content's sums and Gram are read once instead of S times as well, and the multi apply reads its S maps from LDS once per pixel and style.
Part (b), whole videos at 320 x 240 (BASELINE configs[4]'s size), --frames frames, samples 256+256 and 64+128, S in {1, 4, 8}:
video.render_appearance_sweep (one call) against S calls of video.render_video, host clock around calls that end in a device-to-host copy,
alternating, after one discarded round.  Five more repeats of one render_video give the run-to-run spread the S = 1 comparison has to be read
against.
--part trace: the 800 x 800, S = 8 decode alone, a few rounds of M and N and nothing else -- the workload to put under
`rocprofv3 --kernel-trace --stats` (in a run of its own) for the per-kernel times."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GRIDS = [(800, 800), (320, 240)]
STYLES = [1, 4, 8, 16]
med = statistics.median


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3


def decode_inputs(dev, hw, S):
    import crnerf_amd.synth as synth
    st = synth.decoder_state(3, contrast=4000.0)
    w = [torch.from_numpy(st[k]).to(dev) for k in synth.DECODER_SHAPES if not k.endswith(".f")]
    g = torch.Generator(device=dev).manual_seed(hw + S)
    x = torch.rand(hw, 64, device=dev, generator=g)
    styles = [torch.rand(1024, 64, device=dev, generator=g) for _ in range(S)]
    return w, x, styles


def part_a(say, dev, steps, warmup):
    from crnerf_amd import ops
    say("(a) decode only: M = crossray_decode_multi (float planes), U = the same with uint8 frames, N = S x crossray_decode; %d timed rounds M N U after "
        "%d discarded, events around each series; medians in us" % (steps, warmup))
    for W, H in GRIDS:
        hw = W * H
        for S in STYLES:
            w, x, styles = decode_inputs(dev, hw, S)
            t_stats = [timed(lambda: ops.crossray_style_stats(styles, w, hw)) for _ in range(warmup + 5)][warmup:]
            stats = ops.crossray_style_stats(styles, w, hw)
            out_m = torch.empty(S, 3, hw, device=dev)
            out_u = torch.empty(S, hw, 3, dtype=torch.uint8, device=dev)
            out_n = torch.empty(S, 3, hw, device=dev)

            def single():
                for s in range(S):
                    ops.crossray_decode(x, styles[s], w, out=out_n[s])
            series = (("M", lambda: ops.crossray_decode_multi(x, stats, w, out=out_m)), ("N", single),
                      ("U", lambda: ops.crossray_decode_multi(x, stats, w, out=out_u, u8=True)))
            t = {"M": [], "N": [], "U": []}
            for i in range(warmup + steps):
                for name, fn in series:
                    us = timed(fn)
                    if i >= warmup:
                        t[name].append(us)
            same = torch.equal(out_m, out_n) and torch.equal(out_u, (out_n.clamp(0, 1) * 255).to(torch.uint8).permute(0, 2, 1))
            q = np.percentile(t["N"], [25, 75])
            say("%4d x %-4d S %2d: M %8.1f  U %8.1f  N %8.1f (quartiles %.1f .. %.1f)  M/N %.3f  U/N %.3f  apply bytes predict %.3f (float) %.3f (uint8)  "
                "style stats once per sweep %.1f  M per style %.1f  images bit-identical: %s"
                % (W, H, S, med(t["M"]), med(t["U"]), med(t["N"]), q[0], q[1], med(t["M"]) / med(t["N"]), med(t["U"]) / med(t["N"]),
                   (256 + 12 * S) / (268.0 * S), (256 + 3 * S) / (268.0 * S), med(t_stats), med(t["M"]) / S, same))


class HP:
    nerf_out_dim, pertubeCord, N_emb_xyz, N_emb_dir, use_disp, encode_a, encode_random, N_a = 64, False, 15, 4, False, True, True, 48

    def __init__(self, nc, ni):
        self.img_wh, self.N_samples, self.N_importance = [320, 240], nc, ni


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, r


def part_b(say, dev, frames):
    import crnerf_amd.synth as synth
    from crnerf_amd import pipeline, video
    say("(b) videos of %d frames at 320 x 240: render_appearance_sweep (one call) against S x render_video; wall clock in ms around calls that end in "
        "the device-to-host copies; one discarded round, then two timed rounds alternating sweep / videos (both shown)" % frames)
    enc = pipeline.encoder_sameoutputsize(64).to(dev)
    enc.load_state_dict({k: torch.from_numpy(v) for k, v in synth.encoder_state(4, 2.0).items()})
    g = torch.Generator(device=dev).manual_seed(0)
    photos = [torch.rand(1, 3, 100, 100, device=dev, generator=g) for _ in range(8)]
    for nc, ni in ((256, 256), (64, 128)):
        hp = HP(nc, ni)
        m, emb = pipeline.get_model(hp, dev), pipeline.get_embeddings(hp)
        m["coarse"].load_state_dict({k: torch.from_numpy(v) for k, v in synth.mlp_state(1, 3.0, 1.0).items()})
        m["fine"].load_state_dict({k: torch.from_numpy(v) for k, v in synth.mlp_state(2, 3.0, 1.0).items()})
        m["decoder"].load_state_dict({k: torch.from_numpy(v) for k, v in synth.decoder_state(3, contrast=4000.0).items()})
        one = lambda p: video.render_video(m, emb, enc, p, hp, n_frames=frames)  # noqa: E731
        wall(lambda: one(photos[0]))                                             # warm-up: code objects, packs, allocator
        rep = [wall(lambda: one(photos[0]))[0] for _ in range(5)]
        say("%d+%d: five repeats of one render_video: %s ms; median %.1f, spread (max - min) / median %.4f"
            % (nc, ni, ["%.1f" % v for v in rep], med(rep), (max(rep) - min(rep)) / med(rep)))
        for S in (1, 4, 8):
            ts, tv, same = [], [], None
            for i in range(3):
                a, sweep = wall(lambda: video.render_appearance_sweep(m, emb, enc, photos[:S], hp, n_frames=frames))
                b, vids = wall(lambda: [one(p) for p in photos[:S]])
                if i:
                    ts.append(a)
                    tv.append(b)
                same = all(np.array_equal(sweep[s][f], vids[s][f]) for s in range(S) for f in range(frames))
            say("%d+%d S %d: sweep %s ms, %d x render_video %s ms; medians %.1f / %.1f, sweep / videos %.3f (1/S = %.3f), sweep / one video %.3f; "
                "frames byte-identical: %s" % (nc, ni, S, ["%.1f" % v for v in ts], S, ["%.1f" % v for v in tv], med(ts), med(tv), med(ts) / med(tv),
                                              1.0 / S, med(ts) / med(rep), same))
        del m


def part_trace(dev):
    from crnerf_amd import ops
    hw, S = 800 * 800, 8
    w, x, styles = decode_inputs(dev, hw, S)
    stats = ops.crossray_style_stats(styles, w, hw)
    for _ in range(6):
        ops.crossray_decode_multi(x, stats, w)
        ops.crossray_decode_multi(x, stats, w, u8=True)
        for s in range(S):
            ops.crossray_decode(x, styles[s], w)
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="ab", choices=["a", "b", "ab", "trace"])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("appearance_sweep_ab: no GPU -- a timing taken anywhere else says nothing")
    dev = torch.device("cuda:0")
    lines = []

    def say(s):
        lines.append(s)
        print(s, flush=True)
        if a.out:                                   # line by line: a part that fails keeps what was measured before it
            with open(a.out, "a") as f:
                f.write(s + "\n")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").close()
    with torch.no_grad():
        if a.part == "trace":
            part_trace(dev)
            return
        say("device: %s" % torch.cuda.get_device_name(0))
        if "a" in a.part:
            part_a(say, dev, a.steps, a.warmup)
        if "b" in a.part:
            part_b(say, dev, a.frames)


if __name__ == "__main__":
    main()

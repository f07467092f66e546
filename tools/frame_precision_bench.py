"""Frame time of BASELINE configs[2] (one 800 x 800 frame = 640,000 rays in 32,768-ray chunks x (64 + 128), appearance encoder + on-device rays +
render + cross-ray decode) per inference precision, on one GPU in one process: the configs[2] leg of bench.py, event-timed, for an arbitrary list
of precisions and with every run reported (the question "is mode A faster than mode B by more than B's run-to-run spread" needs all of them).

    python tools/frame_precision_bench.py [--precisions bf16,bf16_fc,bf16_hc] [--runs 3] [--frames 3] [--warmup 2] [--out FILE]

The runs of the precisions are interleaved (A B C A B C ...), each run = `warmup` untimed frames of the SAME precision (warm-up = the timed path:
packs cached, LDS limits raised, clocks where this mode puts them) and then `frames` frames between two HIP events.  A precision this build
does not know is reported as skipped (the tool also runs on a checkout that predates a mode)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--precisions", default="bf16,bf16_fc,bf16_hc")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--frames", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import crnerf_amd
    import crnerf_amd.synth as synth
    from crnerf_amd import pipeline

    dev = torch.device("cuda:0")

    class HP:
        nerf_out_dim, pertubeCord, N_emb_xyz, N_emb_dir, use_disp, encode_a, encode_random, N_a = 64, False, 15, 4, False, True, True, 48
        img_wh, N_samples, N_importance = [800, 800], 64, 128
    hp = HP()
    m, emb = pipeline.get_model(hp, dev), pipeline.get_embeddings(hp)
    m["coarse"].load_state_dict({k: torch.from_numpy(v) for k, v in synth.mlp_state(1, 3.0, 1.0).items()})
    m["fine"].load_state_dict({k: torch.from_numpy(v) for k, v in synth.mlp_state(2, 3.0, 1.0).items()})
    m["decoder"].load_state_dict({k: torch.from_numpy(v) for k, v in synth.decoder_state(3).items()})
    enc = pipeline.encoder_sameoutputsize(64).to(dev)
    enc.load_state_dict({k: torch.from_numpy(v) for k, v in synth.encoder_state(4, 2.0).items()})
    focal = 800 / 2 / np.tan(np.pi / 6)
    K = np.array([[focal, 0, 400], [0, focal, 400], [0, 0, 1]])
    c2w = np.array([[1, 0, 0, 0.05], [0, -1, 0, 0.02], [0, 0, -1, 0.1]], dtype=np.float32)
    photo = torch.rand(1, 3, 100, 100, device=dev)

    def known(prec):     # set_precision maps a string it does not know to "f32" (or raises): such a mode does not exist in this build
        before = crnerf_amd.get_precision()
        try:
            crnerf_amd.set_precision(prec)
            return crnerf_amd.get_precision() == prec
        except ValueError:
            return False
        finally:
            crnerf_amd.set_precision(before)

    precs = a.precisions.split(",")
    result = {"workload": "800x800 rays in 32,768-ray chunks x (64+128), appearance encoder + on-device rays + render + cross-ray decode",
              "device": torch.cuda.get_device_name(0), "frames_per_run": a.frames, "warmup_frames_per_run": a.warmup, "ms_per_frame": {}, "skipped": []}
    for p in precs:
        if known(p):
            result["ms_per_frame"][p] = []
        else:
            result["skipped"].append(p)
    with torch.no_grad():
        for _ in range(a.runs):
            for p in result["ms_per_frame"]:
                frame = lambda: pipeline.render_frame(m, emb, enc, photo, 800, 800, K, c2w, hp, chunk=32768, precision=p)  # noqa: E731
                for _ in range(a.warmup):
                    frame()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                for _ in range(a.frames):
                    frame()
                e1.record()
                torch.cuda.synchronize()
                result["ms_per_frame"][p].append(e0.elapsed_time(e1) / a.frames)
    result["summary"] = {p: {"min": min(v), "max": max(v), "spread": max(v) - min(v), "median": sorted(v)[len(v) // 2]} for p, v in result["ms_per_frame"].items()}
    text = json.dumps(result, indent=1, sort_keys=True)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()

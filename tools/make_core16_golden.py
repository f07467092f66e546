"""Records tests/golden/g_core16_parent.npz: what the fp32 core's inference kernels return, bit for bit, on the shapes of
tests/test_gpu_core16_schedule.py.  Run it on the GPU with the library the schedule is to be compared against:

    CRNERF_LIB_PATH=cr-nerf-pytorch_amd/variants/libcrnerf_parent.so python tools/make_core16_golden.py [--out FILE]

(the fixture in the tree was recorded from the build before the sub-stage stagger, csrc/mlp_core16.h LAG).  Inputs come from crnerf_amd.synth
with fixed seeds; the file holds outputs only.  Two cases are periodic in their inputs so that the file stays small: the many-quads render
repeats PERIOD rays and mlp_forward at P = 4096 repeats the 130 rows of the P = 130 case.  Rays and points are independent of each other,
so their outputs repeat as well; this tool verifies that on the recording build and stores one period.  The test module imports its cases and
inputs from here, so both always see the same data."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GOLDEN = os.path.join(ROOT, "tests", "golden", "g_core16_parent.npz")
DEV = "cuda:0"
PERIOD = 12                       # distinct rays of the many-quads case: three quads, so a ray meets every pair of waves
SCHED_CUS = 256                   # the many-quads case is 4 x (256 + 2) rays: more quads than an MI355X has CUs

# name: (R, Nc, Ni, distinct rays)
RENDER_CASES = {
    "one_ragged_quad_1x64+128": (1, 64, 128, 1),
    "two_quads_5x33+31": (5, 33, 31, 5),
    "one_step_passes_4x8+8": (4, 8, 8, 4),
    "coarse_only_4x2+0": (4, 2, 0, 4),
    "coarse_only_4x64+0": (4, 64, 0, 4),
    "more_quads_than_cus_1032x8+8": (4 * (SCHED_CUS + 2), 8, 8, PERIOD),
    "longest_passes_4x256+256": (4, 256, 256, 4),
}
RNG_CASE = ("rng_5x33+31", 5, 33, 31, {"seed": 20240607, "jitter": True, "u": True, "noise": True, "perturb": 1.0})
MLP_CASES = {"mlp_16": (16, 16), "mlp_130": (130, 130), "mlp_4096": (4096, 130)}      # name: (P, distinct rows)
RENDER_KEYS = ["weights_coarse", "feature_coarse", "depth_coarse", "weights_fine", "feature_fine", "depth_fine", "z_fine"]


def packs():
    import crnerf_amd.synth as synth
    from crnerf_amd import ops
    st = [{k: torch.from_numpy(v).to(DEV) for k, v in synth.mlp_state(s, 3.0, 1.0).items()} for s in (5, 6)]
    return ops.pack_mlp_weights(st[0]), ops.pack_mlp_weights(st[1])


def render_inputs(name):
    """(rays[R,8] on the device, keyword arguments of ops.render_rays)."""
    import crnerf_amd.synth as synth
    R, nc, ni, distinct = RENDER_CASES[name] if name in RENDER_CASES else RNG_CASE[1:4] + (RNG_CASE[1],)
    base = synth.rays(distinct, seed=11)
    rays = torch.from_numpy(np.ascontiguousarray(base[np.arange(R) % distinct])).to(DEV)
    kw = dict(z_steps=torch.linspace(0, 1, nc).to(DEV), want_z_fine=True)
    if ni > 0 and name in RENDER_CASES:               # (the rng case draws u in the kernel)
        kw["u"] = torch.linspace(0, 1, ni).to(DEV)
    return rays, kw


def mlp_inputs(name):
    P, distinct = MLP_CASES[name]
    x = np.random.default_rng(7).uniform(-1.0, 1.0, (130, 120)).astype(np.float32)[:distinct]
    return torch.from_numpy(np.ascontiguousarray(x[np.arange(P) % distinct])).to(DEV)


def expand(name, key, arr):
    """A stored array at the case's full size (periodic cases hold one period)."""
    if name in RENDER_CASES:
        R, distinct = RENDER_CASES[name][0], RENDER_CASES[name][3]
        return arr if R == distinct else arr[np.arange(R) % distinct]
    if name in MLP_CASES:
        P, distinct = MLP_CASES[name]
        return arr if P == distinct else arr[np.arange(P) % distinct]
    return arr


def record():
    from crnerf_amd import ops
    pc, pf = packs()
    out = {}

    def keep(name, key, t, distinct):
        a = t.cpu().numpy()
        if a.shape[0] != distinct:
            if not np.array_equal(a, a[np.arange(a.shape[0]) % distinct]):
                raise SystemExit("%s/%s: the recording build's outputs do not repeat with its inputs" % (name, key))
            a = a[:distinct]
        out["%s/%s" % (name, key)] = a

    with torch.no_grad():
        for name, (R, nc, ni, distinct) in RENDER_CASES.items():
            rays, kw = render_inputs(name)
            res = ops.render_rays(pc, pf, rays, nc, ni, **kw)
            torch.cuda.synchronize()
            for k, v in res.items():
                keep(name, k, v, distinct)
        name, R, nc, ni, rng = RNG_CASE
        rays, kw = render_inputs(name)
        res = ops.render_rays(pc, pf, rays, nc, ni, noise_std=1.0, rng=rng, **kw)
        torch.cuda.synchronize()
        for k, v in res.items():
            keep(name, k, v, R)
        for name, (P, distinct) in MLP_CASES.items():
            keep(name, "out", ops.mlp_forward(pc, mlp_inputs(name)), distinct)
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=GOLDEN)
    a = ap.parse_args()
    arrays = record()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    np.savez_compressed(a.out, **arrays)
    print("%s: %d arrays, %d bytes, library %s" % (a.out, len(arrays), os.path.getsize(a.out), os.environ.get("CRNERF_LIB_PATH", "(shipped)")))

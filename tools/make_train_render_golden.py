"""Records tests/golden/g_train_render_parent.json: the SHA-256 of every output and every parameter gradient of a grad-mode render, for each
training mode of crnerf_amd.autograd on shapes small enough to run in milliseconds and large enough to reach every branch of the render node --
so that a change of the node (which rows it keeps, how it gets them back, which packs it shares, which operator its backward calls, when it reads
a setting) that moves one bit of one gradient shows.  Run it on the GPU with the tree whose bytes are the contract (the fixture in the tree was
recorded while autograd.py had three render nodes, FusedRenderFn / MixedRecomputeRenderFn / MixedFusedRenderFn, and every getter read the
environment itself):

    python tools/make_train_render_golden.py [--out FILE]

Inputs: tests/test_gpu_train_fused.py's -- synth.mlp_state(41 / 42, 2.0, 0.5) in two NeRF_sigma modules, synth.rays and depths / uniforms / noise
drawn like its _inputs, and the loss of its _fused_vs_unfused, which reads weights, feature and depth.  Shapes (R, Nc, Ni):
  * "ragged"  (5, 33, 20): a partial ray quad;
  * "single"  (16, 64, 0): one model;
  * "chunks"  (12, 33, 20) with CRNERF_TRAIN_CHUNK_POINTS=212 inside deferred_param_grads(): three chunks of four rays -- the packs shared by the
    chunks of a call, the transposed packs made by the first chunk's backward, the chunks' rng offsets, the deferred sum of the chunks' gradients;
  * "fine_only": "ragged" with feature_fine.sum() as the loss -- the coarse model's 24 gradients are None.
Modes: the four forward modes, each also with recompute; "auto" under the four weight-gradient forms; training precision bf16 stored, recomputed
and recomputed with CRNERF_TRAIN_BF16_UNFUSED=1; render_rays_cross_ray with perturb = 1 and noise_std = 1 after torch.manual_seed(0) (the in-kernel
draws and the tensors the backward composites with) and rng_ray_offset=7; the un-fused training leg (models.rendering._render_unfused(...,
train=True): MlpFn + CompositeFn) in f32 and bf16.  Every mode runs on "ragged"; "chunks" runs the forward modes, the weight-gradient forms and the
bf16 modes.

Every case runs twice in the process; a case whose two runs differ in one byte is left out and named.  Per tensor the file holds the digest and,
for diagnosis, the shape and the largest absolute value.  tests/test_gpu_train_plan.py imports its cases from here, so both always issue the same
calls."""
import argparse
import contextlib
import hashlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GOLDEN = os.path.join(ROOT, "tests", "golden", "g_train_render_parent.json")
DEV = "cuda:0"
SHAPES = {"ragged": (5, 33, 20), "single": (16, 64, 0), "chunks": (12, 33, 20), "fine_only": (5, 33, 20)}
VARIABLES = ("CRNERF_TRAIN_FWD", "CRNERF_TRAIN_FWD_X3", "CRNERF_WGRAD_F32", "CRNERF_WGRAD_BF16X3", "CRNERF_WGRAD_BF16", "CRNERF_TRAIN_BF16",
             "CRNERF_TRAIN_RECOMPUTE", "CRNERF_TRAIN_BF16_UNFUSED", "CRNERF_TRAIN_CHUNK_POINTS")
FORWARDS = ("f32", "f32x3", "f32h2", "auto")
WGRADS = ("f32", "bf16", "bf16x3", "f16x2")
OUTPUTS = ("weights_coarse", "feature_coarse", "depth_coarse", "weights_fine", "feature_fine", "depth_fine")

# mode name: {"forward", "wgrad", "bf16", "recompute": what the four setters are given; "env"; "path": "fused" | "shim" | "unfused"}
MODES = {}
for _f in FORWARDS:
    MODES["fwd_" + _f] = {"forward": _f}
    MODES["fwd_%s+recompute" % _f] = {"forward": _f, "recompute": True}
for _w in WGRADS:
    MODES["auto/wgrad_" + _w] = {"forward": "auto", "wgrad": _w}
MODES["bf16"] = {"bf16": True}
MODES["bf16+recompute"] = {"bf16": True, "recompute": True}
MODES["bf16+recompute/unfused_rebuild"] = {"bf16": True, "recompute": True, "env": {"CRNERF_TRAIN_BF16_UNFUSED": "1"}}
MODES["shim_draws/f32"] = {"forward": "f32", "path": "shim"}
MODES["shim_draws/auto"] = {"forward": "auto", "path": "shim"}
MODES["unfused/f32"] = {"path": "unfused"}
MODES["unfused/bf16"] = {"bf16": True, "path": "unfused"}
ON_CHUNKS = ["fwd_" + _f for _f in FORWARDS] + ["auto/wgrad_" + _w for _w in WGRADS] + ["bf16", "bf16+recompute", "bf16+recompute/unfused_rebuild"]
CASES = [("ragged", m) for m in MODES] + [("single", "defaults"), ("fine_only", "defaults")] + [("chunks", m) for m in ON_CHUNKS]
MODES["defaults"] = {}


def case_name(case):
    return "%s/%s" % case


class _Args:
    nerf_out_dim, img_wh, pertubeCord = 64, [8, 8], False


class Inputs:
    """The two modules and, per shape, what a case reads; made once and left unchanged."""

    def __init__(self):
        import crnerf_amd.synth as synth
        from crnerf_amd.models.nerf import NeRF_sigma, PosEmbedding
        self.args = _Args()
        self.models = {"coarse": NeRF_sigma("coarse", self.args, in_channels_xyz=93, in_channels_dir=27).to(DEV),
                       "fine": NeRF_sigma("fine", self.args, in_channels_xyz=93, in_channels_dir=27, encode_random=True).to(DEV)}
        self.models["coarse"].load_state_dict({k: torch.from_numpy(v) for k, v in synth.mlp_state(41, 2.0, 0.5).items()})
        self.models["fine"].load_state_dict({k: torch.from_numpy(v) for k, v in synth.mlp_state(42, 2.0, 0.5).items()})
        self.emb = {"xyz": PosEmbedding(14, 15), "dir": PosEmbedding(3, 4)}
        C = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)  # noqa: E731
        self.t = {}
        for shape, (R, Nc, Ni) in SHAPES.items():
            rng = np.random.default_rng(3)
            rays = synth.rays(R, seed=3)
            z = np.sort(rng.uniform(rays[:, 6:7], rays[:, 7:8], (R, Nc)).astype(np.float32), -1)
            u = rng.uniform(0, 1, (R, max(Ni, 1))).astype(np.float32)
            self.t[shape] = {"rays": C(rays), "z": C(z), "u": C(u) if Ni else None, "noise_c": C(rng.normal(size=(R, Nc)).astype(np.float32)),
                             "noise_f": C(rng.normal(size=(R, Nc + Ni)).astype(np.float32)) if Ni else None,
                             "gw": torch.randn(R, 64, generator=torch.Generator().manual_seed(1)).to(DEV),
                             "gd": torch.randn(R, generator=torch.Generator().manual_seed(2)).to(DEV)}


@contextlib.contextmanager
def applied(shape, mode):
    """The setters and the environment of one case; both as they were afterwards (the setters at their defaults)."""
    from crnerf_amd import autograd as AG
    env = dict(mode.get("env", {}), **({"CRNERF_TRAIN_CHUNK_POINTS": "212"} if shape == "chunks" else {}))
    before = {k: os.environ.pop(k, None) for k in VARIABLES}
    os.environ.update(env)
    try:
        AG.set_training_forward_precision(mode.get("forward"))
        AG.set_wgrad_precision(mode.get("wgrad"))
        AG.set_training_precision("bf16" if mode.get("bf16") else "f32")
        AG.set_training_recompute(bool(mode.get("recompute")))
        with AG.deferred_param_grads(shape == "chunks"):
            yield
    finally:
        AG.set_training_forward_precision(None)
        AG.set_wgrad_precision(None)
        AG.set_training_precision("f32")
        AG.set_training_recompute(False)
        for k, v in before.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def run_case(inp, case):
    """{tensor name: tensor or None} of one case: the outputs of the render and the gradient of every parameter of both modules."""
    from crnerf_amd import autograd as AG
    from crnerf_amd.models import rendering
    shape, mode_name = case
    mode = MODES[mode_name]
    R, Nc, Ni = SHAPES[shape]
    t, m = inp.t[shape], inp.models
    for mod in m.values():
        mod.zero_grad(set_to_none=True)
    with applied(shape, mode):
        path = mode.get("path", "fused")
        if path == "shim":
            torch.manual_seed(0)
            res = rendering.render_rays_cross_ray(m, inp.emb, t["rays"], None, Nc, False, 1.0, 1.0, Ni, 1 << 20, False, args=inp.args, rng_ray_offset=7)
            out = {k: res[k] for k in OUTPUTS}
        elif path == "unfused":
            out = rendering._render_unfused(m["coarse"], m["fine"], t["rays"], Nc, Ni, False, None, t["z"], t["u"], t["noise_c"], t["noise_f"], 1.0, False,
                                            1 << 20, train=True)
        else:
            out = AG.fused_render_with_grad(m["coarse"], m["fine"] if Ni else None, t["rays"], Nc, Ni, False, None, t["z"], t["u"], t["noise_c"], t["noise_f"], 1.0)
        if shape == "fine_only":
            loss = out["feature_fine"].sum()
        elif Ni == 0:
            loss = 0.5 * (out["feature_coarse"] * t["gw"]).sum() + (out["depth_coarse"] * t["gd"]).sum() + 0.1 * (out["weights_coarse"] ** 2).sum()
        else:
            loss = ((out["feature_fine"] * t["gw"]).sum() + 0.5 * (out["feature_coarse"] * t["gw"]).sum() + (out["depth_fine"] * t["gd"]).sum()
                    + 0.1 * (out["weights_fine"] ** 2).sum())
        loss.backward()                                  # (deferred gradients reach .grad in the callback at the end of this pass)
    torch.cuda.synchronize()
    got = {"out/" + k: v.detach() for k, v in out.items() if torch.is_tensor(v)}
    for tag, mod in m.items():
        for n, p in mod.named_parameters():
            got["grad/%s.%s" % (tag, n)] = None if p.grad is None else p.grad.detach().clone()
    return got


def digest(t):
    """[SHA-256 of the bytes, shape, largest absolute value] of a tensor; None stays None (a gradient nothing was propagated to)."""
    if t is None:
        return None
    host = t.detach().cpu().contiguous()
    return [hashlib.sha256(host.numpy().tobytes()).hexdigest(), list(host.shape), float(host.abs().max()) if host.numel() else 0.0]


def digests(inp, case):
    return {k: digest(v) for k, v in run_case(inp, case).items()}


def record():
    inp = Inputs()
    table, unstable = {}, []
    for case in CASES:
        a, b = digests(inp, case), digests(inp, case)
        if a != b:
            unstable.append((case_name(case), [k for k in a if a[k] != b[k]]))
            continue
        table[case_name(case)] = a
    return table, unstable


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=GOLDEN)
    a = ap.parse_args()
    table, unstable = record()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(table, f, indent=0, sort_keys=True)
        f.write("\n")
    for name, keys in unstable:
        print("NOT RECORDED (two runs differ): %s: %s" % (name, ", ".join(keys)))
    print("%s: %d of %d cases, %d bytes" % (a.out, len(table), len(CASES), os.path.getsize(a.out)))

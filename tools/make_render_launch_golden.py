"""Records tests/golden/g_render_launch_parent.npz: what every kernel variant behind the render and MLP launchers returns, bit for bit, when EVERY
optional field of the argument block is in use -- so that a pointer, stride, count or scheduler slot that the launch layer (csrc/launch.h and the
launchers on top of it) wires to the wrong place shows as a wrong byte.  Run it on the GPU with the library the launch layer is to be compared
against:

    CRNERF_LIB_PATH=path/to/libcrnerf_parent.so python tools/make_render_launch_golden.py [--out FILE]

(the fixture in the tree was recorded from the build before launch.h existed, when every launcher filled its parameter block by hand).

Inputs: one CPU generator with a fixed seed draws the two models' weights (nn.Linear's uniform init: small, so the fp16 cores stay in range) and
every input tensor, each a distinct draw.  A render variant is called in two FORMS per ray count:
  * "all": view_dir, z_steps, a per-ray u [R,Ni], noise_coarse and noise_fine with noise_std = 0.5, use_disp, want_z_fine;
  * "zc":  the same with z_coarse in place of z_steps and a shared u table [Ni] (u_stride = 0);
the in-kernel-draw variants in one form, "draw": the library refuses a drawn quantity that also comes as a tensor, so z_coarse, u and the noises
are left to the kernel and view_dir, z_steps, use_disp and noise_std stay.  Ray counts: R = 6 (two quads, the second partial, static quad map) and
R = 4 * CUs + 6 (more quads than workgroups: the scheduler slot, iters > 1).  The stand-alone MLP entries run on P = 130 points.

The file holds the SHA-256 of every returned tensor except acts_* (those buffers come from torch.empty and have bytes no kernel writes;
tests/test_gpu_train_fused.py and tests/test_gpu_mixed_fused.py cover them), and for the R = 6 cases the arrays themselves, so that a failure names
the first element that differs.  The raw_* rows of the training twins would alone take the file past its 200 KB budget: of those it holds one
CRC-32 per sample point (a failure names the first row).  It also holds the CU count it was recorded on, because the large ray count depends on
it.  The test module imports its cases and inputs from here, so both always issue the same calls.

A second fixture, tests/golden/g_render_entries_parent.npz (--fixture entries), holds the same for the render entries of include/crnerf_lean.h and
include/crnerf_lean_composite.h, which did not exist when the first one was recorded: ENTRY_VARIANTS, on the same Inputs, forms "all" and "zc" and
ray counts.  The fixture in the tree was recorded from the build before csrc/abi.hip described every render entry by one descriptor.  The inputs
keep the fp16 cores in range, so the repair launches behind "auto" and repair_x3= leave at once (tests/test_gpu_lean_composite.py covers the other
side)."""
import argparse
import hashlib
import json
import os
import sys
import zlib

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GOLDEN = os.path.join(ROOT, "tests", "golden", "g_render_launch_parent.npz")
ENTRIES_GOLDEN = os.path.join(ROOT, "tests", "golden", "g_render_entries_parent.npz")
DEV = "cuda:0"
SEED = 20261020
NC, NI, SMALL_R, MLP_P = 5, 4, 6, 130
RNG = {"seed": 977, "ray_offset": 7, "perturb": 1.0, "jitter": True, "u": True, "noise": True}
PRECISIONS = ("f32", "bf16", "f16", "f32x3", "f32h2", "auto")

# name: (precision, keyword arguments of ops.render_rays on top of the form's); "bf16_fine" is ops.render_rays_bf16_fine
RENDER_VARIANTS = {
    "f32": ("f32", {}), "f32_lean": ("f32", {"lean": True}), "bf16": ("bf16", {}), "f16": ("f16", {}), "f32x3": ("f32x3", {}), "f32h2": ("f32h2", {}),
    "auto": ("auto", {}), "bf16_fine": ("bf16", {}),
    "train_f32": ("f32", {"train": True}), "train_bf16": ("bf16", {"train": True}), "train_f32x3": ("f32x3", {"train": True}),
    "train_f32h2": ("f32h2", {"train": True}), "train_auto": ("auto", {"train": True}),
}
DRAW_VARIANTS = {
    "rng_f32": ("f32", {}), "rng_f32x3": ("f32x3", {}), "rng_f32h2": ("f32h2", {}),
    "rng_train_f32": ("f32", {"train": True}), "rng_train_f32x3": ("f32x3", {"train": True}), "rng_train_f32h2": ("f32h2", {"train": True}),
}
SIZES = ("small", "large")
# (variant, form, size) of every render case; (precision, sigma_only) of every MLP case
RENDER_CASES = ([(v, f, s) for v in RENDER_VARIANTS for f in ("all", "zc") for s in SIZES] + [(v, "draw", s) for v in DRAW_VARIANTS for s in SIZES])
MLP_CASES = [(p, so) for p in PRECISIONS for so in (False, True)]
# name: (the ops function, precision, keyword arguments on top of the form's); "x3" as repair_x3 stands for the coarse model's f32x3 pack
ENTRY_VARIANTS = {
    "lean_bf16": ("render_rays", "bf16", {"lean": True}), "lean_f16": ("render_rays", "f16", {"lean": True}),
    "cw_f32h2": ("render_coarse_weights", "f32h2", {}), "cw_f32x3": ("render_coarse_weights", "f32x3", {}), "cw_auto": ("render_coarse_weights", "auto", {}),
    "cw_f16_repair": ("render_coarse_weights", "f16", {"repair_x3": "x3"}),
    "lean_bf16_fine": ("render_rays_bf16_fine", "bf16", {"lean": True}),
}
ENTRY_CASES = [(v, f, s) for v in ENTRY_VARIANTS for f in ("all", "zc") for s in SIZES]


def case_name(case):
    return "/".join(str(c) for c in case)


def device_cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def n_rays(size, cus):
    return SMALL_R if size == "small" else 4 * cus + SMALL_R


class Inputs:
    """Everything the cases read, drawn once, in a fixed order, from one CPU generator (the large tensors are drawn for `cus` CUs)."""

    def __init__(self, cus):
        from crnerf_amd import ops
        g = np.random.default_rng(SEED)
        self.cus = cus
        states = []
        for _ in range(2):
            st = {}
            for name, shape in zip(ops.MLP_TENSOR_NAMES, ops.MLP_TENSOR_SHAPES):
                fan_in = shape[1] if len(shape) == 2 else ops.MLP_TENSOR_SHAPES[ops.MLP_TENSOR_NAMES.index(name.replace("bias", "weight"))][1]
                st[name] = torch.from_numpy((g.uniform(-1.0, 1.0, shape) / np.sqrt(fan_in)).astype(np.float32)).to(DEV)
            states.append(st)
        self.packs = {p: tuple(ops.pack_mlp_weights(st, precision=p) for st in states) for p in PRECISIONS}
        f32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)  # noqa: E731
        self.z_steps = f32(np.sort(g.uniform(0.0, 1.0, NC)))
        self.u_shared = f32(np.sort(g.uniform(0.0, 1.0, NI)))
        self.x = f32(g.uniform(-1.0, 1.0, (MLP_P, 120)))
        self.t = {}
        for size in SIZES:              # the large tensors last: nothing else depends on the CU count
            R = n_rays(size, cus)
            d = g.normal(size=(R, 3))
            d /= np.linalg.norm(d, axis=1, keepdims=True)
            v = g.normal(size=(R, 3))
            v /= np.linalg.norm(v, axis=1, keepdims=True)
            near, far = g.uniform(0.3, 1.0, (R, 1)), g.uniform(3.0, 5.0, (R, 1))
            z_coarse = near + (far - near) * np.sort(g.uniform(0.0, 1.0, (R, NC)), axis=1)
            self.t[size] = {
                "rays": f32(np.concatenate([g.normal(0.0, 0.1, (R, 3)), d, near, far], axis=1)), "view_dir": f32(v), "z_coarse": f32(z_coarse),
                "u_rays": f32(np.sort(g.uniform(0.0, 1.0, (R, NI)), axis=1)), "noise_coarse": f32(g.normal(size=(R, NC))),
                "noise_fine": f32(g.normal(size=(R, NC + NI))), "weights_coarse": f32(g.uniform(0.0, 0.3, (R, NC))),
            }


def run_render(inp, case):
    """The returned dict of one render case."""
    from crnerf_amd import ops
    variant, form, size = case
    t = inp.t[size]
    kw = dict(use_disp=True, view_dir=t["view_dir"], noise_std=0.5, want_z_fine=True)
    if form == "draw":
        precision, extra = DRAW_VARIANTS[variant]
        kw.update(z_steps=inp.z_steps, rng=dict(RNG), **extra)
    else:
        precision, extra = RENDER_VARIANTS[variant]
        kw.update(noise_fine=t["noise_fine"], **extra)
        kw.update(dict(z_steps=inp.z_steps, u=t["u_rays"]) if form == "all" else dict(z_coarse=t["z_coarse"], u=inp.u_shared))
    pc, pf = inp.packs[precision]
    with torch.no_grad():
        if variant == "bf16_fine":
            res = ops.render_rays_bf16_fine(pf, t["rays"], t["weights_coarse"], NC, NI, **kw)
        else:
            if form != "draw":
                kw["noise_coarse"] = t["noise_coarse"]
            res = ops.render_rays(pc, pf, t["rays"], NC, NI, precision=precision, **kw)
    torch.cuda.synchronize()
    return {k: v for k, v in res.items() if not k.startswith("acts_")}


def run_entry(inp, case):
    """The returned dict of one case of ENTRY_VARIANTS: every optional input the entry reads is in use."""
    from crnerf_amd import ops
    variant, form, size = case
    fn, precision, extra = ENTRY_VARIANTS[variant]
    t = inp.t[size]
    pc, pf = inp.packs[precision]
    kw = dict(use_disp=True, noise_std=0.5, **extra)
    kw.update(dict(z_steps=inp.z_steps) if form == "all" else dict(z_coarse=t["z_coarse"]))
    with torch.no_grad():
        if fn == "render_coarse_weights":
            if kw.get("repair_x3") == "x3":
                kw["repair_x3"] = inp.packs["f32x3"][0]
            res = ops.render_coarse_weights(pc, t["rays"], NC, precision=precision, noise_coarse=t["noise_coarse"], **kw)
        else:
            kw.update(view_dir=t["view_dir"], noise_fine=t["noise_fine"], want_z_fine=True, u=t["u_rays"] if form == "all" else inp.u_shared)
            if fn == "render_rays_bf16_fine":
                res = ops.render_rays_bf16_fine(pf, t["rays"], t["weights_coarse"], NC, NI, **kw)
            else:
                res = ops.render_rays(pc, pf, t["rays"], NC, NI, precision=precision, noise_coarse=t["noise_coarse"], **kw)
    torch.cuda.synchronize()
    return res


def run_mlp(inp, case):
    from crnerf_amd import ops
    precision, sigma_only = case
    with torch.no_grad():
        out = ops.mlp_forward(inp.packs[precision][0], inp.x[:, :93].contiguous() if sigma_only else inp.x, sigma_only=sigma_only, precision=precision)
    torch.cuda.synchronize()
    return {"out": out}


def words(t):
    """A returned tensor as int32 words on the host: the bytes compare, so NaNs do too."""
    return np.ascontiguousarray(t.detach().cpu().contiguous().view(torch.int32).numpy())


def sha(w):
    return hashlib.sha256(w.tobytes()).hexdigest()


def row_crcs(w):
    """One CRC-32 per sample point of a raw_* tensor [R,N,65]."""
    return np.array([zlib.crc32(r.tobytes()) for r in w.reshape(-1, w.shape[-1])], dtype=np.uint32)


def stored(key, w):
    """What the fixture keeps of an R = 6 output."""
    return row_crcs(w) if key.startswith("raw_") else w


def _record_cases(inp, cases, run, shas, arrays):
    for case in cases:
        for k, v in run(inp, case).items():
            w = words(v)
            shas["%s/%s" % (case_name(case), k)] = sha(w)
            if case[2] == "small":
                arrays["%s/%s" % (case_name(case), k)] = stored(k, w)


def record_entries():
    cus = device_cus()
    shas, arrays = {}, {}
    _record_cases(Inputs(cus), ENTRY_CASES, run_entry, shas, arrays)
    arrays["meta"] = np.array(json.dumps({"cus": cus, "sha256": shas}, sort_keys=True))
    return arrays


def record():
    cus = device_cus()
    inp = Inputs(cus)
    shas, arrays = {}, {}
    _record_cases(inp, RENDER_CASES, run_render, shas, arrays)
    for case in MLP_CASES:
        for k, v in run_mlp(inp, case).items():
            shas["mlp/%s/%s" % (case_name(case), k)] = sha(words(v))
    arrays["meta"] = np.array(json.dumps({"cus": cus, "sha256": shas}, sort_keys=True))
    return arrays


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--fixture", choices=("launch", "entries"), default="launch")
    ap.add_argument("--out")
    a = ap.parse_args()
    a.out = a.out or (GOLDEN if a.fixture == "launch" else ENTRIES_GOLDEN)
    arrays = record() if a.fixture == "launch" else record_entries()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    np.savez_compressed(a.out, **arrays)
    size = os.path.getsize(a.out)
    if size >= 200 * 1000:
        raise SystemExit("%s: %d bytes, the fixture's budget is 200 KB" % (a.out, size))
    print("%s: %d arrays, %d bytes, %d CUs, library %s" % (a.out, len(arrays) - 1, size, device_cus(), os.environ.get("CRNERF_LIB_PATH", "(shipped)")))

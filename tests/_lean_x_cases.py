"""Inputs of tests/test_gpu_lean_x.py (the lean render on the x3 / h2 cores, include/crnerf_lean_x.h): the two trained-like models, their packs, a full
set of caller-side tensors for a shape, and the constructions that make the h2 range guard trip -- on the coarse side, on the fine side, and in the
pack itself.  Everything is built once per process and never modified."""
import numpy as np
import torch

import crnerf_amd.synth as synth
from crnerf_amd import ops

DEV = "cuda:0"
ST_C, ST_F = synth.mlp_state(5, 3.0, 1.0), synth.mlp_state(6, 3.0, 1.0)      # tests/test_gpu_lean_pair.py's states; largest |weight| 1.2


def C(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


_AUTO = {}


def auto_pack(key, state=None):
    """The AutoPack (h2 + x3) of a state, packed once per key; "c" / "f": ST_C / ST_F."""
    if key not in _AUTO:
        st = {"c": ST_C, "f": ST_F}.get(key, state)
        _AUTO[key] = ops.pack_mlp_weights({k: C(v) for k, v in st.items()}, precision="auto")
        assert _AUTO[key].h2 is not None, key
    return _AUTO[key]


def packs(precision, coarse="c", fine="f"):
    """(coarse pack, fine pack) for "f32x3" / "f32h2" / "auto" of two packed states."""
    pc, pf = auto_pack(coarse), auto_pack(fine)
    return {"auto": (pc, pf), "f32h2": (pc.h2, pf.h2), "f32x3": (pc.x3, pf.x3)}[precision]


def inputs(R, nc, ni, disp, seed=4):
    """(rays, keywords) with every optional tensor in use: jittered ascending coarse depths, per-ray uniforms, density noise of both passes with
    noise_std = 1, and a view direction of its own."""
    rays = synth.rays(R, seed=3)
    rng = np.random.default_rng(seed)
    vd = rng.normal(size=(R, 3)).astype(np.float32)
    vd /= np.linalg.norm(vd, axis=-1, keepdims=True)
    kw = dict(use_disp=disp, view_dir=C(vd), z_coarse=C(np.sort(rng.uniform(rays[:, 6:7], rays[:, 7:8], (R, nc)).astype(np.float32), -1)),
              u=C(rng.uniform(0, 1, (R, ni)).astype(np.float32)), noise_coarse=C(rng.normal(size=(R, nc)).astype(np.float32)),
              noise_fine=C(rng.normal(size=(R, nc + ni)).astype(np.float32)), noise_std=1.0, want_z_fine=True)
    return C(rays), kw


def overflow_state():
    """tests/test_gpu_h2.py's overflow net with one more amplifying layer: hidden unit 0 of xyz_encoding_1 / _2 / _3 multiplies the raw x coordinate by
    250 * 250 * 4, so h2 and h3 -- operands of layers 3 and 4 -- pass 65,504 where x is of ordinary size; every weight packs for the h2 core (|w| < 255)."""
    st = dict(synth.mlp_state(5, 1.0))
    for layer, gain in ((1, 250.0), (2, 250.0), (3, 4.0)):
        w = st["xyz_encoding_%d.0.weight" % layer].copy()
        w[0, 0] = gain
        st["xyz_encoding_%d.0.weight" % layer] = w
    return st


def overflow_rays():
    """256 rays; the first 192 have tiny origins and depths and stay inside fp16's range under overflow_state(), many of the other 64 leave it."""
    rays = synth.rays(256, seed=3, H=16, W=16).copy()
    rays[:192, 0:3] *= 1e-3
    rays[:192, 6] = 1e-4
    rays[:192, 7] = 2e-3
    return C(rays)


def flagged_pack():
    """An AutoPack of overflow_state() with one weight of 300: the h2 pack carries the range flag (crnerf_pack_mlp_weights_h2_async), x3 is as ever."""
    big = overflow_state()
    w = big["xyz_encoding_4.0.weight"].copy()
    w[7, 9] = 300.0
    big["xyz_encoding_4.0.weight"] = w
    return ops.pack_mlp_weights_auto({k: C(v) for k, v in big.items()}, check=False)

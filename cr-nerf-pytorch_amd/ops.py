"""Tensor-level wrappers over the C ABI: allocate outputs with torch, enqueue the HIP kernels on the
current stream.  Every function here runs on the GPU or raises."""
import collections
import ctypes
import math
import os

import numpy as np
import torch

from . import _lib
from .precision import resolve

MLP_TENSOR_NAMES = (
    [n for i in range(1, 9) for n in ("xyz_encoding_%d.0.weight" % i, "xyz_encoding_%d.0.bias" % i)]
    + ["xyz_encoding_final.weight", "xyz_encoding_final.bias", "static_sigma.0.weight", "static_sigma.0.bias",
       "dir_encoding.0.weight", "dir_encoding.0.bias", "static_rgb.0.weight", "static_rgb.0.bias"])
MLP_TENSOR_SHAPES = (
    [(256, 93), (256,)] + [(256, 256), (256,)] * 3 + [(256, 349), (256,)] + [(256, 256), (256,)] * 3
    + [(256, 256), (256,), (1, 256), (1,), (128, 283), (128,), (64, 128), (64,)])


def _wlist(weights, name):
    """The parameter tensors of a call as they are (fp32, contiguous: checked; no detach -- they are only asked for their address and their shape,
    and a training step passes ~450 of them)."""
    return [t if (t.dtype == torch.float32 and t.is_contiguous()) else _f32c(t.detach(), name) for t in weights]


def _slots_valid(slots):
    for d, name, q in slots:
        if d.get(name) is not q:
            return False
    return True


def cached_params(module):
    """tuple(module.parameters()) looked up once: nn.Module.parameters() walks the module tree on every call, and the grad-mode
    checks of the shim modules ran it ~6,000 generator steps per training step (1-2 ms of host time at the reference's 1,024-ray
    batch, where the step is host-bound).  The cache remembers WHERE each Parameter lives (the owning sub-module's _parameters
    dict and its name) and every lookup re-checks those slots by identity, so anything that swaps a Parameter object --
    load_state_dict(assign=True), `layer.weight = nn.Parameter(...)`, to_empty() / meta materialisation,
    torch.__future__.set_overwrite_module_params_on_conversion -- rebuilds it instead of leaving stale tensors behind."""
    c = module.__dict__.get("_crnerf_pcache")
    if c is None or not _slots_valid(c[0]):
        slots = tuple((m._parameters, name, q) for m in module.modules() for name, q in m._parameters.items() if q is not None)
        c = (slots, tuple(s[2] for s in slots))
        module.__dict__["_crnerf_pcache"] = c
    return c[1]


_LIST_CACHE = os.environ.get("CRNERF_LIST_CACHE", "1") != "0"      # 0: measurement switch (A/B of the host time)


def cached_list(module, key, build):
    """A list of a module's Parameter objects (or sub-modules) in kernel order, looked up once per module and generation of the parameter slots
    (cached_params' identity check: a swapped Parameter rebuilds it).  The training step asked for these lists ~20 times per step through 570
    attribute lookups (round 6: the 1,024-ray step is host-bound).  Parameters and modules only -- a cached VIEW would be one autograd node
    shared by every use in a step, and the uses' gradients would then be summed in the engine's order instead of use by use."""
    if not _LIST_CACHE:
        return build()
    cached_params(module)
    tag = module.__dict__["_crnerf_pcache"]
    store = module.__dict__.setdefault("_crnerf_lists", {})
    c = store.get(key)
    if c is None or c[0] is not tag:
        c = (tag, build())
        store[key] = c
    return c[1]


def any_requires_grad(module):
    for q in cached_params(module):
        if q.requires_grad:
            return True
    return False


def mlp_params(module):
    """The 24 NeRF_sigma parameters in MLP_TENSOR_NAMES order; cached with the same slot-identity check as cached_params."""
    c = module.__dict__.get("_crnerf_mlp_params")
    if c is None or not _slots_valid(c[0]):
        slots = []
        for n in MLP_TENSOR_NAMES:
            path, _, leaf = n.rpartition(".")
            owner = module.get_submodule(path)
            slots.append((owner._parameters, leaf, owner._parameters[leaf]))
        c = (tuple(slots), tuple(s[2] for s in slots))
        module.__dict__["_crnerf_mlp_params"] = c
    return c[1]


def _f32c(t, name):
    if t.dtype != torch.float32 or not t.is_contiguous():
        t = t.to(torch.float32).contiguous()
    if not t.is_cuda:
        raise RuntimeError("crnerf_amd: %s is on %s; the HIP path needs GPU tensors and has no CPU fallback" % (name, t.device))
    return t


class AutoPack:
    """The packs of precision="auto": `h2` (None when crnerf_pack_mlp_weights_h2 refused the weights: one of them is >= 255 or not finite) and
    `x3`, the scale-free fallback (always there)."""
    __slots__ = ("h2", "x3")

    def __init__(self, h2, x3):
        self.h2, self.x3 = h2, x3


class PackRangeError(RuntimeError):
    """crnerf_pack_mlp_weights_f16 refused the weights: one of them is not finite or beyond fp16's 65,504."""


class F16Pack:
    """An f16 pack.  It has the bf16 pack's size, so unlike the other layouts it cannot be told from one by its length: the type is the tag (`data`: the
    uint8 buffer)."""
    __slots__ = ("data",)

    def __init__(self, data):
        self.data = data

    def data_ptr(self):
        return self.data.data_ptr()

    def numel(self):
        return self.data.numel()


# One record per arithmetic a kernel family exists for (precision.CORES): the library's entry points BY NAME (looked up on the loaded library, so
# importing this module does not load it), `tag`, the type a pack of that core has where its byte size cannot tell it from another's, and the entries
# of the lean render (crnerf.h; crnerf_lean.h for the pair core's two builds) and of the coarse-weights render (crnerf_lean_composite.h): None where
# the core has none.
_Core = collections.namedtuple("_Core", "bytes pack forward render render_train tag render_lean coarse_weights")
_CORES = {
    "f32": _Core("crnerf_packed_mlp_bytes", "crnerf_pack_mlp_weights", "crnerf_mlp_forward_f32", "crnerf_render_rays_f32", "crnerf_render_rays_train_f32", None,
                 "crnerf_render_rays_lean_f32", None),
    "bf16": _Core("crnerf_packed_mlp_bf16_bytes", "crnerf_pack_mlp_weights_bf16", "crnerf_mlp_forward_bf16", "crnerf_render_rays_bf16",
                  "crnerf_render_rays_train_bf16", None, "crnerf_render_rays_lean_bf16", None),
    # one-piece fp16 operands: a point whose operands leave fp16's range comes out as NaN; inference only
    "f16": _Core("crnerf_packed_mlp_f16_bytes", "crnerf_pack_mlp_weights_f16", "crnerf_mlp_forward_f16", "crnerf_render_rays_f16", None, F16Pack,
                 "crnerf_render_rays_lean_f16", "crnerf_render_coarse_weights_f16"),
    # fp32 on the bf16 matrix cores: every weight as three bf16 pieces, k-step-major fragment stream; six MFMAs per product
    "f32x3": _Core("crnerf_packed_mlp_x3_bytes", "crnerf_pack_mlp_weights_x3", "crnerf_mlp_forward_f32x3", "crnerf_render_rays_f32x3",
                   "crnerf_render_rays_train_f32x3", None, None, "crnerf_render_coarse_weights_f32x3"),
    # fp32 on the fp16 matrix cores: every weight, scaled by 2^8, as two fp16 pieces; three MFMAs per product
    "f32h2": _Core("crnerf_packed_mlp_h2_bytes", "crnerf_pack_mlp_weights_h2", "crnerf_mlp_forward_f32h2", "crnerf_render_rays_f32h2",
                   "crnerf_render_rays_train_f32h2", None, None, "crnerf_render_coarse_weights_f32h2"),
}


def _check_pack(lib, name, packed):
    """The packed layouts differ in size (the f16 one in type), so a mix-up is caught here instead of rendering garbage."""
    if packed is None:
        return
    core = _CORES[name]
    if core.tag is not None:
        if not isinstance(packed, core.tag):
            raise ValueError("crnerf_amd: the %s entry points need packs from pack_mlp_weights(..., precision=%r)" % (name, name))
        return
    if isinstance(packed, F16Pack):
        raise ValueError("crnerf_amd: an f16 pack was handed to the %s entry points (it has the bf16 pack's size and another element type)" % name)
    got, want = packed.numel() * packed.element_size(), getattr(lib, core.bytes)()
    if got != want:
        raise ValueError("crnerf_amd: packed weights are %d bytes, the %s entry points need %d (pack with precision=%r)" % (got, name, want, name))


def _mlp_tensor_list(state):
    tensors = []
    for name, shape in zip(MLP_TENSOR_NAMES, MLP_TENSOR_SHAPES):
        t = state[name]
        if tuple(t.shape) != shape:
            raise ValueError("crnerf_amd: %s has shape %s, the HIP kernels are built for %s "
                             "(D=8, W=256, N_emb_xyz=15, N_emb_dir=4, nerf_out_dim=64)" % (name, tuple(t.shape), shape))
        tensors.append(t if (t.dtype == torch.float32 and t.is_contiguous() and t.is_cuda) else _f32c(t.detach(), name))
    return tensors


def _pack(state, bytes_fn, pack_fn, out=None, range_ok=False):
    """The 24 tensors of `state` (mapping name -> device tensor, models/nerf.py:137-154) through the library's `pack_fn` into `out` (default: a new
    buffer of `bytes_fn`() bytes).  range_ok: None instead of an error when the library refuses the weights' range (CRNERF_ERR_RANGE)."""
    lib = _lib.load()
    tensors = _mlp_tensor_list(state)
    if out is None:
        out = torch.empty(getattr(lib, bytes_fn)(), dtype=torch.uint8, device=tensors[0].device)
    rc = getattr(lib, pack_fn)(_lib.ptr_array(tensors, "mlp tensor"), ctypes.c_void_p(out.data_ptr()), _lib.stream_ptr())
    if rc == _lib.ERR_RANGE and range_ok:
        return None
    _lib.check(rc, pack_fn)
    return out


def pack_mlp_weights_auto(state, check=True):
    """check=False (training: a pack per optimiser step): crnerf_pack_mlp_weights_h2_async -- no wait for the stream; a refused pack carries its verdict
    as a flag word the h2 kernels read on the device (they then leave everything to the f32x3 repair), so `h2` is never None."""
    core = _CORES["f32h2"]
    h2 = _pack(state, core.bytes, core.pack, range_ok=True) if check else _pack(state, core.bytes, "crnerf_pack_mlp_weights_h2_async")
    return AutoPack(h2, pack_mlp_weights_x3(state))


def pack_h2_in_range(packed_h2):
    """True when the h2 / transposed-h2 pack carries no range flag (crnerf_pack_h2_status; waits for the stream)."""
    lib = _lib.load()
    rc = lib.crnerf_pack_h2_status(ctypes.c_void_p(packed_h2.data_ptr()), _lib.stream_ptr())
    if rc == _lib.ERR_RANGE:
        return False
    _lib.check(rc, "crnerf_pack_h2_status")
    return True


def pack_mlp_weights(state, out=None, precision="f32"):
    """state: mapping name -> device tensor with the 24 NeRF_sigma tensors (models/nerf.py:137-154).
    precision "f32" -> buffer for the *_f32 entry points, "bf16" -> for the *_bf16 ones, "f16" -> for the *_f16 ones (the bf16 layout with fp16
    elements; PackRangeError when a weight does not fit fp16), "f32x3" / "f32h2" -> for the *_f32x3 / *_f32h2 ones
    (pack_mlp_weights_x3 / pack_mlp_weights_h2; different layouts each), "auto" -> an AutoPack (h2 + x3)."""
    name = resolve(precision)
    if out is not None and name in ("auto", "f32x3", "f32h2"):
        raise ValueError("crnerf_amd: out= is for the f32 / bf16 packs")
    if name == "auto":
        return pack_mlp_weights_auto(state)
    core = _CORES[name]
    if name != "f16":
        return _pack(state, core.bytes, core.pack, out)
    out = _pack(state, core.bytes, core.pack, out, range_ok=True)
    if out is None:
        msg = _lib.load().crnerf_last_error()
        raise PackRangeError("%s failed (code %d): %s" % (core.pack, _lib.ERR_RANGE, msg.decode() if msg else "?"))
    return F16Pack(out)


def pack_mlp_weights_x3(state):
    """Packed weights for the "f32x3" entry points (include/crnerf.h): every weight as three bf16 pieces, k-step-major fragment stream."""
    return _pack(state, *_CORES["f32x3"][:2])


def mlp_forward_x3(packed_x3, x, sigma_only=False):
    """NeRF_sigma.forward in fp32 on the bf16 matrix cores (three-piece splits, six MFMAs per product; crnerf_mlp_forward_f32x3)."""
    return mlp_forward(packed_x3, x, sigma_only=sigma_only, precision="f32x3")


def pack_mlp_weights_h2(state):
    """Packed weights for the "f32h2" entry points (include/crnerf.h): every weight, scaled by 2^8, as two fp16 pieces."""
    return _pack(state, *_CORES["f32h2"][:2])


def mlp_forward_h2(packed_h2, x, sigma_only=False):
    """NeRF_sigma.forward in fp32 on the fp16 matrix cores (two-piece splits, three MFMAs per product; crnerf_mlp_forward_f32h2)."""
    return mlp_forward(packed_h2, x, sigma_only=sigma_only, precision="f32h2")


def render_rays_x3(packed_coarse, packed_fine, rays, n_samples, n_importance, **kw):
    """render_rays(..., precision="f32x3")."""
    return render_rays(packed_coarse, packed_fine, rays, n_samples, n_importance, precision="f32x3", **kw)


def pack_mlp_weights_t(state):
    """Transposed fragment stream for the backward-data kernel."""
    return _pack(state, "crnerf_packed_mlp_t_bytes", "crnerf_pack_mlp_weights_t")


def mlp_forward_train(packed, x):
    """Forward that keeps the layer activations.  Returns (out[n,65], acts)."""
    lib = _lib.load()
    x = _f32c(x, "x")
    n = x.shape[0]
    out = torch.empty(n, 65, dtype=torch.float32, device=x.device)
    acts = torch.empty(lib.crnerf_mlp_train_acts_bytes(n), dtype=torch.uint8, device=x.device)
    _lib.check(lib.crnerf_mlp_forward_train_f32(ctypes.c_void_p(packed.data_ptr()), _lib.dev_ptr(x), _lib.dev_ptr(out),
                                                ctypes.c_void_p(acts.data_ptr()), n, _lib.stream_ptr()), "crnerf_mlp_forward_train_f32")
    return out, acts


def pack_mlp_weights_t_x3(state):
    """Transposed x3 fragment stream for the backward-data kernel on the x3 core (crnerf_mlp_backward_x3_f32)."""
    return _pack(state, "crnerf_packed_mlp_t_x3_bytes", "crnerf_pack_mlp_weights_t_x3")


def pack_mlp_weights_t_h2(state):
    """Transposed h2 fragment stream for the backward-data kernel on the h2 core (crnerf_mlp_backward_h2_f32): two fp16 pieces of 2^8 w.  No range
    check of its own -- pack_mlp_weights_h2 / pack_mlp_weights(..., precision="auto") of the same weights is the check."""
    return _pack(state, "crnerf_packed_mlp_t_h2_bytes", "crnerf_pack_mlp_weights_t_h2")


BWD_PHASE_DGRAD, BWD_PHASE_WGRAD = 8, 16      # CRNERF_BWD_PHASE_* (include/crnerf.h)


def mlp_backward(packed_t, x, out, d_out, acts, wgrad_bf16=False, dgrad_x3=False, dgrad_h2=False, fallback_t_x3=None, phase=None, scratch=None, grads=None):
    """Gradients of sum(out * d_out) w.r.t. the 24 tensors, in MLP_TENSOR_NAMES order.  wgrad_bf16: True / 1 = CRNERF_BWD_WGRAD_BF16
    (include/crnerf.h) -- the weight gradients of every Linear except static_sigma from bf16-rounded operands; 2 / "x3" =
    CRNERF_BWD_WGRAD_BF16X3 -- fp32-accurate weight gradients of the 256 x 256 blocks from three-piece bf16 splits on the bf16 matrix
    cores; 3 / "f16x2" (dgrad_h2 only) = CRNERF_BWD_WGRAD_F16X2 -- the same with the full 256 x 256 blocks from two-piece fp16 splits (three
    piece products, the h2 core's arithmetic; bf16x3 takes over by itself where an operand leaves fp16's range).  Data gradients as the dgrad_*
    arguments say; biases and everything else exact fp32.
    phase: None = the whole backward; "dgrad" = CRNERF_BWD_PHASE_DGRAD (returns the scratch tensor that holds the deltas; x may be None);
    "wgrad" = CRNERF_BWD_PHASE_WGRAD on `scratch` (the tensor a "dgrad" call returned; packed_t / out / d_out may be None) -- the two halves may
    be enqueued on different streams, ordered by the caller (autograd.FusedRenderFn)."""
    lib = _lib.load()
    do_d, do_w = phase != "wgrad", phase != "dgrad"
    if phase not in (None, "dgrad", "wgrad"):
        raise ValueError("crnerf_amd: mlp_backward phase is None, 'dgrad' or 'wgrad', got %r" % (phase,))
    x = _f32c(x, "x") if (do_w or x is not None) else None
    out, d_out = (_f32c(out, "out"), _f32c(d_out, "d_out")) if do_d else (None, None)
    n = x.shape[0] if x is not None else out.shape[0]
    dev = x.device if x is not None else out.device
    f16x2 = wgrad_bf16 in (3, "f16x2", "h2")
    if f16x2 and not dgrad_h2:
        raise ValueError("crnerf_amd: f16x2 weight gradients take their delta ranges from the h2 data gradient (dgrad_h2=True)")
    if do_w and grads is None:
        grads = [torch.empty(s, dtype=torch.float32, device=dev) for s in MLP_TENSOR_SHAPES]
    need = lib.crnerf_mlp_train_scratch_bytes(n)
    if scratch is None:
        if phase == "wgrad":
            raise ValueError("crnerf_amd: mlp_backward(phase='wgrad') needs the scratch of the 'dgrad' call")
        scratch = torch.empty(need, dtype=torch.uint8, device=dev)
    elif scratch.numel() < need or not scratch.is_contiguous() or scratch.dtype != torch.uint8:
        raise ValueError("crnerf_amd: mlp_backward scratch must be a contiguous uint8 tensor of >= %d bytes" % need)
    # dgrad_x3 / dgrad_h2: the data gradient on the x3 / h2 core; packed_t is then a pack_mlp_weights_t_x3 / pack_mlp_weights_t_h2 pack
    fn, name, want = ((lib.crnerf_mlp_backward_h2_f32, "crnerf_mlp_backward_h2_f32", lib.crnerf_packed_mlp_t_h2_bytes()) if dgrad_h2 else
                      (lib.crnerf_mlp_backward_x3_f32, "crnerf_mlp_backward_x3_f32", lib.crnerf_packed_mlp_t_x3_bytes()) if dgrad_x3 else
                      (lib.crnerf_mlp_backward_ex_f32, "crnerf_mlp_backward_ex_f32", lib.crnerf_packed_mlp_t_bytes()))
    if do_d and packed_t.numel() != want:
        raise ValueError("crnerf_amd: %s needs a %d-byte transposed pack, got %d" % (name, want, packed_t.numel()))
    if fallback_t_x3 is not None and (not dgrad_h2 or fallback_t_x3.numel() != lib.crnerf_packed_mlp_t_x3_bytes()):
        raise ValueError("crnerf_amd: fallback_t_x3 is the pack_mlp_weights_t_x3 safety net of dgrad_h2")
    nul = ctypes.c_void_p(None)
    head = (ctypes.c_void_p(packed_t.data_ptr()) if do_d else nul,) + ((ctypes.c_void_p(fallback_t_x3.data_ptr() if (fallback_t_x3 is not None and do_d) else None),) if dgrad_h2 else ())
    flags = 4 if f16x2 else (2 if wgrad_bf16 in (2, "x3", "bf16x3") else (1 if wgrad_bf16 else 0))
    flags |= BWD_PHASE_DGRAD if phase == "dgrad" else (BWD_PHASE_WGRAD if phase == "wgrad" else 0)
    _lib.check(fn(*head, _lib.dev_ptr(x) if x is not None else nul, _lib.dev_ptr(out) if do_d else nul, _lib.dev_ptr(d_out) if do_d else nul,
                  ctypes.c_void_p(acts.data_ptr()), ctypes.c_void_p(scratch.data_ptr()),
                  _lib.ptr_array(grads, "grad") if do_w else None, n, flags, _lib.stream_ptr()), name)
    return scratch if phase == "dgrad" else grads


def pack_mlp_weights_mixed(state):
    """bf16 B-operand fragment streams of every nn.Linear (forward and transposed) for the mixed-precision training twins
    (crnerf_mlp_*_mixed_f32, include/crnerf.h).  Returns (packed, tensors): the twins also read the fp32 biases / sigma head."""
    return _pack(state, "crnerf_packed_mlp_mixed_bytes", "crnerf_pack_mlp_weights_mixed"), _mlp_tensor_list(state)


def mlp_forward_train_mixed(packed_mixed, tensors, x):
    """Mixed-precision forward that keeps the layer activations (bf16 rows, kernel-internal order).  Returns (out[n,65], acts)."""
    lib = _lib.load()
    x = _f32c(x, "x")
    n = x.shape[0]
    out = torch.empty(n, 65, dtype=torch.float32, device=x.device)
    acts = torch.empty(lib.crnerf_mlp_train_mixed_acts_bytes(n), dtype=torch.uint8, device=x.device)
    _lib.check(lib.crnerf_mlp_forward_train_mixed_f32(_lib.ptr_array(tensors, "mlp tensor"), ctypes.c_void_p(packed_mixed.data_ptr()), _lib.dev_ptr(x),
                                                      _lib.dev_ptr(out), ctypes.c_void_p(acts.data_ptr()), n, _lib.stream_ptr()),
               "crnerf_mlp_forward_train_mixed_f32")
    return out, acts


def mlp_backward_mixed(packed_mixed, tensors, x, out, d_out, acts, fused_acts=False):
    """Gradients of sum(out * d_out) w.r.t. the 24 tensors through the mixed-precision twins (MLP_TENSOR_NAMES order).
    fused_acts: `acts` was written by the fused renderer's training twin (render_rays(..., precision="bf16", train=True)); x is unused then."""
    lib = _lib.load()
    out, d_out = _f32c(out, "out"), _f32c(d_out, "d_out")
    n = out.shape[0]
    grads = [torch.empty(s, dtype=torch.float32, device=out.device) for s in MLP_TENSOR_SHAPES]
    scratch = torch.empty(lib.crnerf_mlp_train_mixed_scratch_bytes(n), dtype=torch.uint8, device=out.device)
    if fused_acts:
        _lib.check(lib.crnerf_mlp_backward_mixed_ex_f32(_lib.ptr_array(tensors, "mlp tensor"), ctypes.c_void_p(packed_mixed.data_ptr()), _lib.dev_ptr(out),
                                                        _lib.dev_ptr(d_out), ctypes.c_void_p(acts.data_ptr()), ctypes.c_void_p(scratch.data_ptr()),
                                                        _lib.ptr_array(grads, "grad"), n, 1, _lib.stream_ptr()), "crnerf_mlp_backward_mixed_ex_f32")
        return grads
    x = _f32c(x, "x")
    _lib.check(lib.crnerf_mlp_backward_mixed_f32(_lib.ptr_array(tensors, "mlp tensor"), ctypes.c_void_p(packed_mixed.data_ptr()), _lib.dev_ptr(x),
                                                 _lib.dev_ptr(out), _lib.dev_ptr(d_out), ctypes.c_void_p(acts.data_ptr()),
                                                 ctypes.c_void_p(scratch.data_ptr()), _lib.ptr_array(grads, "grad"), n, _lib.stream_ptr()),
               "crnerf_mlp_backward_mixed_f32")
    return grads


def posenc(x, n_freqs):
    lib = _lib.load()
    x = _f32c(x, "x")
    if x.dim() != 2 or x.shape[1] != 3:
        raise ValueError("posenc expects [n,3], got %s" % (tuple(x.shape),))
    out = torch.empty(x.shape[0], 6 * n_freqs + 3, dtype=torch.float32, device=x.device)
    _lib.check(lib.crnerf_posenc_f32(_lib.dev_ptr(x), _lib.dev_ptr(out), x.shape[0], n_freqs, _lib.stream_ptr()), "crnerf_posenc_f32")
    return out


def embed_points(rays, z, dir_emb):
    """x[R*N,120] = cat(PosEmbedding_xyz(o + d z), dir_emb repeated) in one pass (rendering.py:100-114); dir_emb = posenc(dirs, 4)."""
    lib = _lib.load()
    rays, z, dir_emb = _f32c(rays, "rays"), _f32c(z, "z"), _f32c(dir_emb, "dir_emb")
    R, N = z.shape
    if tuple(rays.shape) != (R, 8) or tuple(dir_emb.shape) != (R, 27):
        raise ValueError("embed_points expects rays [R,8], z [R,N], dir_emb [R,27]; got %s %s %s" % (tuple(rays.shape), tuple(z.shape), tuple(dir_emb.shape)))
    x = torch.empty(R * N, 120, dtype=torch.float32, device=z.device)
    _lib.check(lib.crnerf_embed_points_f32(_lib.dev_ptr(rays), _lib.dev_ptr(z), _lib.dev_ptr(dir_emb), _lib.dev_ptr(x), R, N, _lib.stream_ptr()),
               "crnerf_embed_points_f32")
    return x


def mlp_forward_auto(pack, x, sigma_only=False):
    """mlp_forward(..., precision="auto")."""
    return mlp_forward(pack, x, sigma_only=sigma_only, precision="auto")


def mlp_forward(packed, x, sigma_only=False, precision="f32"):
    """NeRF_sigma.forward on the core `precision` names.  "auto" (an AutoPack): the h2 core, then crnerf_mlp_forward_f32x3_repair over the same
    output -- the 128-point groups in which a point left fp16's range are evaluated again on the scale-free x3 core (nothing else is touched; no host
    round trip).  A refused h2 pack: x3 throughout."""
    name = resolve(precision)
    lib = _lib.load()
    x = _f32c(x, "x")
    want = 93 if sigma_only else 120
    if x.dim() != 2 or x.shape[1] != want:
        raise ValueError("mlp_forward expects [n,%d], got %s" % (want, tuple(x.shape)))
    repair = None
    if name == "auto":
        name, packed, repair = ("f32x3", packed.x3, None) if packed.h2 is None else ("f32h2", packed.h2, packed.x3)
    _check_pack(lib, name, packed)
    out = torch.empty(x.shape[0], 1 if sigma_only else 65, dtype=torch.float32, device=x.device)
    tail = (_lib.dev_ptr(x), _lib.dev_ptr(out), x.shape[0], int(bool(sigma_only)))
    fn = _CORES[name].forward
    _lib.check(getattr(lib, fn)(ctypes.c_void_p(packed.data_ptr()), *tail, _lib.stream_ptr()), fn)
    if repair is not None:
        _lib.check(lib.crnerf_mlp_forward_f32x3_repair(ctypes.c_void_p(repair.data_ptr()), *tail, _lib.stream_ptr()), "crnerf_mlp_forward_f32x3_repair")
    return out


_SIGMA_QUERY = {"f32": ("crnerf_sigma_points_f32", "crnerf_sigma_grid_f32"), "bf16": ("crnerf_sigma_points_bf16", "crnerf_sigma_grid_bf16")}   # include/crnerf_geometry.h


def _sigma_query_core(precision, what):
    try:
        name = resolve(precision)
    except ValueError:
        name = None
    if name not in _SIGMA_QUERY:
        raise ValueError("crnerf_amd: %s runs under precision 'f32' or 'bf16', got %r (the other cores have no density query)" % (what, precision))
    return name


def _sigma_input(t, name, what, points=False, on_device=True):
    """A float32, contiguous device tensor of the right rank, as it is: nothing is converted or copied.  on_device=False: the rank alone."""
    if not torch.is_tensor(t):
        raise TypeError("crnerf_amd: %s: %s must be a tensor" % (what, name))
    if points and (t.dim() != 2 or t.shape[1] != 3):
        raise ValueError("crnerf_amd: %s expects %s as [n,3], got %s" % (what, name, tuple(t.shape)))
    if not points and t.dim() != 1:
        raise ValueError("crnerf_amd: %s expects the axis %s as [n], got %s" % (what, name, tuple(t.shape)))
    return _lib.dev_ptr(t, name) if on_device else None


def sigma_points(packed, xyz, precision="f32"):
    """sigma [n] of the model behind `packed` (pack_mlp_weights(..., precision)) at xyz [n,3]: one launch that reads the coordinates, embeds them in
    registers and walks the weight stream up to the sigma head (include/crnerf_geometry.h).  precision "f32": bit-identical to
    mlp_forward(packed, posenc(xyz, 15), sigma_only=True)[:, 0]; "bf16": the bf16 matrix cores with the fused renderer's embedding.
    Domain: |coordinate| < 64 (not checked here: crnerf_amd.geometry checks what it is handed on the host)."""
    name = _sigma_query_core(precision, "sigma_points")
    xp = _sigma_input(xyz, "xyz", "sigma_points", points=True)
    lib = _lib.load()
    _check_pack(lib, name, packed)
    out = torch.empty(xyz.shape[0], dtype=torch.float32, device=xyz.device)
    fn = _SIGMA_QUERY[name][0]
    _lib.check(getattr(lib, fn)(ctypes.c_void_p(packed.data_ptr()), xp, _lib.dev_ptr(out), xyz.shape[0], _lib.stream_ptr()), fn)
    return out


_FEATURE_QUERY = {"f32": "crnerf_feature_points_f32", "bf16": "crnerf_feature_points_bf16"}   # csrc/crnerf_point_features.h (staged)


def feature_points(packed, xyz, dirs, precision="f32", want_sigma=True):
    """(feature [n,64], sigma [n] or None) of the model behind `packed` (pack_mlp_weights(..., precision)) at xyz [n,3] seen from dirs [n,3]: one
    launch that reads the point and its direction, builds both embeddings in registers and walks the whole weight stream
    (csrc/crnerf_point_features.h).  feature rows are pixel-major: what crossray_decode reads in place.  precision "f32": bit-identical to
    mlp_forward(packed, cat(posenc(xyz, 15), posenc(dirs, 4)))[:, :64] and [:, 64]; "bf16": the bf16 matrix cores with the fused renderer's
    embeddings.  want_sigma=False: sigma is not stored and None is returned for it.  dirs are taken as given (not normalised).
    Domain: |coordinate| < 64, for points and directions (not checked)."""
    what = "feature_points"
    name = _sigma_query_core(precision, what)
    for t, n in ((xyz, "xyz"), (dirs, "dirs")):      # every shape before any device
        _sigma_input(t, n, what, points=True, on_device=False)
    if xyz.shape[0] != dirs.shape[0]:
        raise ValueError("crnerf_amd: feature_points: xyz has %d rows and dirs has %d; a direction per point" % (xyz.shape[0], dirs.shape[0]))
    xp, dp = _sigma_input(xyz, "xyz", what, points=True), _sigma_input(dirs, "dirs", what, points=True)      # (both on the current device)
    n = xyz.shape[0]
    feature = torch.empty(n, 64, dtype=torch.float32, device=xyz.device)
    sigma = torch.empty(n, dtype=torch.float32, device=xyz.device) if want_sigma else None
    if n == 0:
        return feature, sigma
    lib = _lib.load()
    _check_pack(lib, name, packed)
    fn = _FEATURE_QUERY[name]
    _lib.check(getattr(lib, fn)(ctypes.c_void_p(packed.data_ptr()), xp, dp, _lib.dev_ptr(feature), _lib.dev_ptr(sigma), n, _lib.stream_ptr()), fn)
    return feature, sigma


def sigma_grid(packed, xs, ys, zs, precision="f32", out=None):
    """sigma [nz, ny, nx] at the nodes (xs[ix], ys[iy], zs[iz]) of the grid the three axis tensors span (any values: non-uniform grids and slabs of
    a larger grid are grids) -- sigma_points without the point list: 4 bytes per point leave, the axes are all that is read.  out=: a contiguous
    float32 [nz, ny, nx] tensor on the axes' device to write into (a slab of a larger volume, say); it is returned.  At most 2^31 - 1 points a call."""
    name = _sigma_query_core(precision, "sigma_grid")
    for t, n in ((xs, "xs"), (ys, "ys"), (zs, "zs")):      # every shape before any device
        _sigma_input(t, n, "sigma_grid", on_device=False)
    ptrs = [_sigma_input(t, n, "sigma_grid") for t, n in ((xs, "xs"), (ys, "ys"), (zs, "zs"))]
    shape = (zs.shape[0], ys.shape[0], xs.shape[0])
    if shape[0] * shape[1] * shape[2] > 2 ** 31 - 1:      # (the library refuses it too; an axis beyond int32 would not reach it intact)
        raise ValueError("crnerf_amd: sigma_grid: %d x %d x %d is more than 2^31 - 1 points in one call (slabs of a grid are grids)" % shape[::-1])
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=xs.device)
    elif not torch.is_tensor(out) or tuple(out.shape) != shape:
        raise ValueError("crnerf_amd: sigma_grid: out must be [nz, ny, nx] = %s, got %s" % (shape, tuple(out.shape) if torch.is_tensor(out) else type(out)))
    op = _lib.dev_ptr(out, "out")
    lib = _lib.load()
    _check_pack(lib, name, packed)
    fn = _SIGMA_QUERY[name][1]
    _lib.check(getattr(lib, fn)(ctypes.c_void_p(packed.data_ptr()), *ptrs, shape[2], shape[1], shape[0], op, _lib.stream_ptr()), fn)
    return out


def mesh_grid(sigma, xs, ys, zs, threshold, normals=True):
    """The iso-surface sigma == threshold of a density grid as an indexed triangle mesh, extracted on the device (include/crnerf_mesh.h states every
    rule: marching tetrahedra on the Kuhn split, inside = sigma > threshold, one shared vertex per active edge, faces oriented out of the dense
    region, content and order deterministic).  sigma [nz, ny, nx] and the axes xs [nx], ys [ny], zs [nz]: float32, contiguous, on the device, as
    they are.  Returns (vertices [V,3] float32, faces [F,3] int32, normals [V,3] float32 or None).
    Count, ONE read-back of the two totals (the only synchronisation), allocate, emit.  The axes are taken to be strictly increasing -- that is what
    the orientation promise rests on -- and this is NOT checked here: crnerf_amd.geometry checks what it is handed."""
    if not torch.is_tensor(sigma):
        raise TypeError("crnerf_amd: mesh_grid: sigma must be a tensor")
    if sigma.dim() != 3:
        raise ValueError("crnerf_amd: mesh_grid expects sigma as [nz, ny, nx], got %s" % (tuple(sigma.shape),))
    for t, n in ((xs, "xs"), (ys, "ys"), (zs, "zs")):      # every shape before any device
        _sigma_input(t, n, "mesh_grid", on_device=False)
    shape = (zs.shape[0], ys.shape[0], xs.shape[0])
    if tuple(sigma.shape) != shape:
        raise ValueError("crnerf_amd: mesh_grid: sigma must be [nz, ny, nx] = %s for these axes, got %s" % (shape, tuple(sigma.shape)))
    if shape[0] * shape[1] * shape[2] > 2 ** 31 - 1:
        raise ValueError("crnerf_amd: mesh_grid: %d x %d x %d is more than 2^31 - 1 nodes in one call" % shape[::-1])
    threshold = float(threshold)
    sp = _lib.dev_ptr(sigma, "sigma")
    ptrs = [_sigma_input(t, n, "mesh_grid") for t, n in ((xs, "xs"), (ys, "ys"), (zs, "zs"))]
    lib = _lib.load()
    dims = (shape[2], shape[1], shape[0])
    dev = sigma.device
    workspace = torch.empty(max(int(lib.crnerf_mesh_workspace_bytes(*dims)), 8), dtype=torch.uint8, device=dev)
    counts = torch.empty(2, dtype=torch.int64, device=dev)
    wp, st = ctypes.c_void_p(workspace.data_ptr()), _lib.stream_ptr()
    _lib.check(lib.crnerf_mesh_count_f32(sp, *dims, threshold, wp, ctypes.c_void_p(counts.data_ptr()), st), "crnerf_mesh_count_f32")
    V, F = counts.tolist()
    if V > 2 ** 31 - 1 or F > 2 ** 31 - 1:
        raise ValueError("crnerf_amd: mesh_grid: %d vertices and %d faces do not fit int32 indices; extract slabs of the grid" % (V, F))
    vertices = torch.empty(V, 3, dtype=torch.float32, device=dev)
    faces = torch.empty(F, 3, dtype=torch.int32, device=dev)
    nrm = torch.empty(V, 3, dtype=torch.float32, device=dev) if normals else None
    if V or F:
        _lib.check(lib.crnerf_mesh_emit_f32(sp, *ptrs, *dims, threshold, wp, V, F, ctypes.c_void_p(vertices.data_ptr()),
                                            ctypes.c_void_p(nrm.data_ptr()) if normals else None, ctypes.c_void_p(faces.data_ptr()), st),
                   "crnerf_mesh_emit_f32")
    return vertices, faces, nrm


def _parts_input(t, name, what, dtype, cols=None, rows=None, on_device=True):
    """An indexed-mesh tensor of the right rank, dtype and row count, contiguous and on the device, as it is.  on_device=False: shape and dtype
    alone -- those refusals need no device."""
    if not torch.is_tensor(t):
        raise TypeError("crnerf_amd: %s: %s must be a tensor" % (what, name))
    if (t.dim() != 1) if cols is None else (t.dim() != 2 or t.shape[1] != cols):
        raise ValueError("crnerf_amd: %s expects %s as %s, got %s" % (what, name, "[n]" if cols is None else "[n,%d]" % cols, tuple(t.shape)))
    if rows is not None and t.shape[0] != rows:
        raise ValueError("crnerf_amd: %s: %s must have %d rows, got %d" % (what, name, rows, t.shape[0]))
    if t.dtype != dtype:
        raise TypeError("crnerf_amd: %s must be %s, got %s" % (name, dtype, t.dtype))
    return _lib.dev_ptr(t, name, dtype) if on_device else None


def _parts_workspace(lib, V, F, dev):
    return torch.empty(max(int(lib.crnerf_mesh_parts_workspace_bytes(V, F)), 16), dtype=torch.uint8, device=dev)


def mesh_parts(faces, n_vertices):
    """The connected parts of an indexed triangle list, labelled on the device (include/crnerf_mesh_parts.h states every rule: parts by shared
    vertex over the valid faces, ids 0..K-1 ascending in the part's smallest vertex id, content deterministic).  faces [F,3]: int32, contiguous, on
    the device, as it is; n_vertices: V.  Returns (vertex_part [V] int32, face_part [F] int32 -- -1 for a face with an id outside [0, V) --,
    part_vertices [K] int32, part_faces [K] int32).  Label, ONE read-back of K (the only synchronisation), allocate, sizes."""
    V = int(n_vertices)
    if V < 0 or V > 2 ** 31 - 1:
        raise ValueError("crnerf_amd: mesh_parts: n_vertices must lie in [0, 2^31 - 1], got %d" % V)
    fp = _parts_input(faces, "faces", "mesh_parts", torch.int32, cols=3)
    F, dev = faces.shape[0], faces.device
    lib = _lib.load()
    vertex_part = torch.empty(V, dtype=torch.int32, device=dev)
    face_part = torch.full((F,), -1, dtype=torch.int32, device=dev) if V == 0 else torch.empty(F, dtype=torch.int32, device=dev)
    K = 0
    st = _lib.stream_ptr()
    p = lambda t: ctypes.c_void_p(t.data_ptr())      # noqa: E731
    if V:
        workspace = _parts_workspace(lib, V, F, dev)
        counts = torch.empty(1, dtype=torch.int64, device=dev)
        _lib.check(lib.crnerf_mesh_parts_label_i32(fp, V, F, p(workspace), p(vertex_part), p(face_part), p(counts), st), "crnerf_mesh_parts_label_i32")
        K = int(counts.item())
    part_vertices = torch.empty(K, dtype=torch.int32, device=dev)
    part_faces = torch.empty(K, dtype=torch.int32, device=dev)
    if K:
        _lib.check(lib.crnerf_mesh_parts_sizes_i32(p(vertex_part), p(face_part), V, F, K, p(part_vertices), p(part_faces), st), "crnerf_mesh_parts_sizes_i32")
    return vertex_part, face_part, part_vertices, part_faces


def mesh_select(vertices, faces, normals, vertex_part, face_part, keep):
    """The mesh minus the parts keep[] does not name (include/crnerf_mesh_parts.h, Selection): kept rows copied byte for byte in their original
    order, ids renumbered by rank.  vertices [V,3] float32, faces [F,3] int32, normals [V,3] float32 or None, vertex_part [V] / face_part [F]
    int32 (what mesh_parts returned), keep [K] uint8 or bool: contiguous, on the device, as they are.  Returns (vertices', faces', normals' or
    None).  Count, ONE read-back of V' and F' (the only synchronisation), allocate, emit."""
    what = "mesh_select"
    vp_ = np_ = fp = vpp = fpp = None
    for on_device in (False, True):      # every shape and dtype before any device
        vp_ = _parts_input(vertices, "vertices", what, torch.float32, cols=3, on_device=on_device)
        V = vertices.shape[0]
        fp = _parts_input(faces, "faces", what, torch.int32, cols=3, on_device=on_device)
        F = faces.shape[0]
        np_ = None if normals is None else _parts_input(normals, "normals", what, torch.float32, cols=3, rows=V, on_device=on_device)
        if not torch.is_tensor(keep) or keep.dtype not in (torch.uint8, torch.bool):
            raise TypeError("crnerf_amd: mesh_select: keep must be a uint8 or bool tensor")
        if keep.dim() != 1:
            raise ValueError("crnerf_amd: mesh_select expects keep as [K], got %s" % (tuple(keep.shape),))
        K = keep.shape[0]
        if K > V:
            raise ValueError("crnerf_amd: mesh_select: keep names %d parts, more than the %d vertices" % (K, V))
        vpp = _parts_input(vertex_part, "vertex_part", what, torch.int32, rows=V, on_device=on_device)
        fpp = _parts_input(face_part, "face_part", what, torch.int32, rows=F, on_device=on_device)
    kp = _lib.dev_ptr(keep, "keep", keep.dtype)      # (a bool tensor is one byte an element, 0 or 1)
    dev = vertices.device
    lib = _lib.load()
    st = _lib.stream_ptr()
    p = lambda t: ctypes.c_void_p(t.data_ptr())      # noqa: E731
    Vk = Fk = 0
    if V and K:
        workspace = _parts_workspace(lib, V, F, dev)
        counts = torch.empty(2, dtype=torch.int64, device=dev)
        _lib.check(lib.crnerf_mesh_parts_select_count(vpp, fpp, V, F, K, kp, p(workspace), p(counts), st), "crnerf_mesh_parts_select_count")
        Vk, Fk = counts.tolist()
    out_v = torch.empty(Vk, 3, dtype=torch.float32, device=dev)
    out_f = torch.empty(Fk, 3, dtype=torch.int32, device=dev)
    out_n = None if normals is None else torch.empty(Vk, 3, dtype=torch.float32, device=dev)
    if Vk or Fk:
        _lib.check(lib.crnerf_mesh_parts_select_emit_f32(vp_, np_, fp, vpp, fpp, V, F, K, kp, p(workspace), Vk, Fk, p(out_v),
                                                         None if out_n is None else p(out_n), p(out_f), st), "crnerf_mesh_parts_select_emit_f32")
    return out_v, out_f, out_n


def _cluster_grid(lo, cell, n, what):
    """(lo, cell as float32-rounded floats, n as ints) of a clustering grid, held to what the library accepts: no device is needed."""
    try:
        exact = all(int(v) == v for v in n)
        lo, cell, n = [float(v) for v in lo], [float(v) for v in cell], [int(v) for v in n]
    except (TypeError, ValueError):
        lo = cell = n = ()
        exact = False
    if len(lo) != 3 or len(cell) != 3 or len(n) != 3 or not exact:
        raise ValueError("crnerf_amd: %s expects lo and cell as 3-sequences of floats and n as a 3-sequence of ints" % what)
    lo, cell = [ctypes.c_float(v).value for v in lo], [ctypes.c_float(v).value for v in cell]      # what the library is handed
    for v in cell:
        if not (math.isfinite(v) and v > 0.0 and math.isfinite(ctypes.c_float(1.0 / v).value)):
            raise ValueError("crnerf_amd: %s: cell must be finite and > 0 as float32, with a finite reciprocal; got %r" % (what, cell))
    for v in lo:
        if not math.isfinite(v):
            raise ValueError("crnerf_amd: %s: lo must be finite as float32, got %r" % (what, lo))
    if min(n) < 1 or max(n) > 2 ** 20:
        raise ValueError("crnerf_amd: %s: n must hold 1 to 2^20 cells on every axis, got %r" % (what, n))
    if n[0] * n[1] * n[2] > 2 ** 31 - 1:
        raise ValueError("crnerf_amd: %s: n = %d x %d x %d is more than 2^31 - 1 cells" % (what, n[0], n[1], n[2]))
    return lo, cell, n


def mesh_cluster(vertices, faces, lo, cell, n, normals=None, colors=None):
    """The mesh simplified by vertex clustering on the device (csrc/crnerf_mesh_simplify.h states every rule: one vertex per occupied cell of the
    n[0] x n[1] x n[2] grid of cell-sized cells whose first corner is lo; cluster ids ascending in the smallest member id; positions, normals and
    colours from exact integer sums; collapsed faces dropped, of the faces over the same three clusters the first kept; content deterministic).
    vertices [V,3] float32, faces [F,3] int32, normals / colors [V,3] float32 or None: contiguous, on the device, as they are; lo, cell:
    3-sequences of floats (rounded to float32); n: 3 ints.  Returns (vertices' [V',3], faces' [F',3], normals' or None, colors' or None,
    vertex_cluster [V] int32).  Count, ONE read-back of V' and F' (the only synchronisation), allocate, emit."""
    what = "mesh_cluster"
    vp_ = fp = np_ = cp = None
    for on_device in (False, True):      # every shape and dtype before any device
        vp_ = _parts_input(vertices, "vertices", what, torch.float32, cols=3, on_device=on_device)
        V = vertices.shape[0]
        fp = _parts_input(faces, "faces", what, torch.int32, cols=3, on_device=on_device)
        F = faces.shape[0]
        np_ = None if normals is None else _parts_input(normals, "normals", what, torch.float32, cols=3, rows=V, on_device=on_device)
        cp = None if colors is None else _parts_input(colors, "colors", what, torch.float32, cols=3, rows=V, on_device=on_device)
        if not on_device:
            lo, cell, n = _cluster_grid(lo, cell, n, what)
    dev = vertices.device
    lib = _lib.load()
    st = _lib.stream_ptr()
    p = lambda t: ctypes.c_void_p(t.data_ptr())      # noqa: E731
    grid = lo + cell + n
    vertex_cluster = torch.empty(V, dtype=torch.int32, device=dev)
    Vk = Fk = 0
    if V:
        workspace = torch.empty(max(int(lib.crnerf_mesh_cluster_workspace_bytes(V, F, n[0] * n[1] * n[2])), 16), dtype=torch.uint8, device=dev)
        counts = torch.empty(2, dtype=torch.int64, device=dev)
        _lib.check(lib.crnerf_mesh_cluster_count_f32(vp_, fp, V, F, *grid, p(workspace), p(vertex_cluster), p(counts), st), "crnerf_mesh_cluster_count_f32")
        Vk, Fk = counts.tolist()
    out_v = torch.empty(Vk, 3, dtype=torch.float32, device=dev)
    out_f = torch.empty(Fk, 3, dtype=torch.int32, device=dev)
    out_n = None if normals is None else torch.empty(Vk, 3, dtype=torch.float32, device=dev)
    out_c = None if colors is None else torch.empty(Vk, 3, dtype=torch.float32, device=dev)
    if Vk or Fk:
        _lib.check(lib.crnerf_mesh_cluster_emit_f32(vp_, np_, cp, fp, p(vertex_cluster), V, F, *grid, p(workspace), Vk, Fk, p(out_v),
                                                    None if out_n is None else p(out_n), None if out_c is None else p(out_c), p(out_f), st),
                   "crnerf_mesh_cluster_emit_f32")
    return out_v, out_f, out_n, out_c, vertex_cluster


def _smooth_scalars(lo, k, steps, lam, mu, what):
    """(lo as float32-rounded floats, k, steps, lam, mu) of a smoothing call, held to what the library accepts: no device is needed."""
    try:
        lo = [float(v) for v in lo]
    except (TypeError, ValueError):
        lo = []
    if len(lo) != 3:
        raise ValueError("crnerf_amd: %s expects lo as a 3-sequence of floats" % what)
    lo = [ctypes.c_float(v).value for v in lo]      # what the library is handed
    if not all(math.isfinite(v) for v in lo):
        raise ValueError("crnerf_amd: %s: lo must be finite as float32, got %r" % (what, lo))
    for name, v in (("k", k), ("steps", steps)):
        if isinstance(v, bool) or int(v) != v:
            raise ValueError("crnerf_amd: %s: %s must be an int, got %r" % (what, name, v))
    k, steps = int(k), int(steps)
    if not -100 <= k <= 100:
        raise ValueError("crnerf_amd: %s: k must lie in [-100, 100], got %d" % (what, k))
    if not 0 <= steps <= 65536:
        raise ValueError("crnerf_amd: %s: steps must lie in [0, 65536], got %d" % (what, steps))
    lam, mu = float(lam), float(mu)
    for name, v in (("lam", lam), ("mu", mu)):
        if not (math.isfinite(v) and abs(v) <= 2.0):
            raise ValueError("crnerf_amd: %s: %s must be finite with |%s| <= 2, got %r" % (what, name, name, v))
    return lo, k, steps, lam, mu


def mesh_smooth(vertices, faces, lo, k, steps, lam, mu, pin_border=True):
    """The vertices after `steps` steps of Taubin's lambda | mu smoothing on the device (csrc/crnerf_mesh_smooth.h states every rule: positions
    on the 2^30 lattice of the box lo, lo + 2^(30 - k); per pass every vertex moves by the weight times the way to the mean of its neighbour
    entries, a pass with lam then a pass with mu per step; vertices without a face, and with pin_border the vertices of an open border, stay;
    content deterministic and independent of the order of the faces).  vertices [V,3] float32, faces [F,3] int32: contiguous, on the device,
    as they are; lo: a 3-sequence of floats (rounded to float32); k, steps: ints; lam, mu: floats.  Returns vertices' [V,3] float32; steps = 0
    is the quantisation round trip.  No read-back."""
    what = "mesh_smooth"
    vp_ = fp = None
    for on_device in (False, True):      # every shape and dtype before any device
        vp_ = _parts_input(vertices, "vertices", what, torch.float32, cols=3, on_device=on_device)
        fp = _parts_input(faces, "faces", what, torch.int32, cols=3, on_device=on_device)
        if not on_device:
            lo, k, steps, lam, mu = _smooth_scalars(lo, k, steps, lam, mu, what)
    V, F, dev = vertices.shape[0], faces.shape[0], vertices.device
    out = torch.empty(V, 3, dtype=torch.float32, device=dev)
    if V:
        lib = _lib.load()
        st = _lib.stream_ptr()
        workspace = torch.empty(max(int(lib.crnerf_mesh_smooth_workspace_bytes(V, F)), 16), dtype=torch.uint8, device=dev)
        wp = ctypes.c_void_p(workspace.data_ptr())
        _lib.check(lib.crnerf_mesh_adjacency_i32(fp, V, F, wp, st), "crnerf_mesh_adjacency_i32")
        _lib.check(lib.crnerf_mesh_smooth_f32(vp_, V, F, *lo, k, steps, lam, mu, 1 if pin_border else 0, wp, ctypes.c_void_p(out.data_ptr()), st),
                   "crnerf_mesh_smooth_f32")
    return out


def mesh_vertex_normals(vertices, faces, k2):
    """Area-weighted vertex normals from the faces, on the device (csrc/crnerf_mesh_smooth.h, Face normals per vertex: the float64 cross product
    of every valid face, times 2^k2, rounded to a 64-bit integer and added to its three corners; the sums normalised in float64; the zero vector
    for a vertex no face uses).  vertices [V,3] float32, faces [F,3] int32: contiguous, on the device, as they are; k2: an int in [-300, 300].
    Returns normals [V,3] float32.  No read-back."""
    what = "mesh_vertex_normals"
    vp_ = fp = None
    for on_device in (False, True):
        vp_ = _parts_input(vertices, "vertices", what, torch.float32, cols=3, on_device=on_device)
        fp = _parts_input(faces, "faces", what, torch.int32, cols=3, on_device=on_device)
        if not on_device:
            if isinstance(k2, bool) or int(k2) != k2 or not -300 <= int(k2) <= 300:
                raise ValueError("crnerf_amd: %s: k2 must be an int in [-300, 300], got %r" % (what, k2))
            k2 = int(k2)
    V, F, dev = vertices.shape[0], faces.shape[0], vertices.device
    out = torch.empty(V, 3, dtype=torch.float32, device=dev)
    if V:
        lib = _lib.load()
        # (F = 0: the neighbour list lies last in the workspace, and the normals do not use it)
        workspace = torch.empty(max(int(lib.crnerf_mesh_smooth_workspace_bytes(V, 0)), 16), dtype=torch.uint8, device=dev)
        _lib.check(lib.crnerf_mesh_vertex_normals_f32(vp_, fp, V, F, k2, ctypes.c_void_p(workspace.data_ptr()), ctypes.c_void_p(out.data_ptr()),
                                                      _lib.stream_ptr()), "crnerf_mesh_vertex_normals_f32")
    return out


def _photo_views(cams, dims, offsets, total_pixels, z_near, what, on_device):
    """The three view tables of csrc/crnerf_mesh_photo.h held to their shapes and dtypes, total_pixels and z_near to what the library accepts.
    Returns (cams, dims, offsets pointers or None, N, total_pixels, z_near)."""
    cp = _parts_input(cams, "cams", what, torch.float64, cols=16, on_device=on_device)
    N = cams.shape[0]
    dp = _parts_input(dims, "dims", what, torch.int32, cols=2, rows=N, on_device=on_device)
    op = _parts_input(offsets, "offsets", what, torch.int64, rows=N, on_device=on_device)
    if isinstance(total_pixels, bool) or int(total_pixels) != total_pixels or not 0 <= int(total_pixels) <= 2 ** 40:
        raise ValueError("crnerf_amd: %s: total_pixels must be an int in [0, 2^40], got %r" % (what, total_pixels))
    z_near = float(z_near)
    if not (math.isfinite(z_near) and z_near > 0.0):
        raise ValueError("crnerf_amd: %s: z_near must be finite and > 0, got %r" % (what, z_near))
    return cp, dp, op, N, int(total_pixels), z_near


def mesh_zbuffer(vertices, faces, cams, dims, offsets, total_pixels, z_near):
    """The z-buffer of an indexed mesh in N posed pinhole views, on the device (csrc/crnerf_mesh_photo.h states every rule: corners projected in
    float64, screen coordinates on a 1/16-pixel lattice, coverage by exact integer edge functions with an inclusive test, perspective-correct
    depth along the optical axis through an atomic minimum; no near-plane clipping, no culling; a view whose table entry does not fit the
    buffer is skipped; content deterministic and independent of the order of the faces).  vertices [V,3] float32, faces [F,3] int32,
    cams [N,16] float64 (fx, fy, cx, cy, R row-major, t), dims [N,2] int32 (W, H), offsets [N] int64: contiguous, on the device, as they are;
    total_pixels: an int; z_near: a float > 0.  Returns the flat float32 depth [total_pixels], +inf where nothing is drawn.  No read-back."""
    what = "mesh_zbuffer"
    vp_ = fp = tables = None
    for on_device in (False, True):      # every shape and dtype before any device
        vp_ = _parts_input(vertices, "vertices", what, torch.float32, cols=3, on_device=on_device)
        fp = _parts_input(faces, "faces", what, torch.int32, cols=3, on_device=on_device)
        tables = _photo_views(cams, dims, offsets, total_pixels, z_near, what, on_device)
    cp, dp, op, N, total, z_near = tables
    depth = torch.empty(total, dtype=torch.float32, device=vertices.device)
    if total:
        _lib.check(_lib.load().crnerf_mesh_zbuffer_f32(vp_, fp, vertices.shape[0], faces.shape[0], cp, dp, op, N, total, z_near,
                                                       ctypes.c_void_p(depth.data_ptr()), _lib.stream_ptr()), "crnerf_mesh_zbuffer_f32")
    return depth


def mesh_photo_colors(vertices, normals, photos, depth, cams, dims, offsets, total_pixels, z_near, depth_tol):
    """Per-vertex colours by reprojection of N posed photos, on the device (csrc/crnerf_mesh_photo.h states every rule: a view counts for a
    vertex when the vertex is in front of it, faces it -- normals given and not zero --, projects inside the photo and is not behind the
    z-buffer by more than the factor 1 + depth_tol; the photo is sampled bilinearly in float64 and the samples are averaged from exact integer
    sums; content deterministic).  vertices [V,3] float32, normals [V,3] float32 or None, photos [total_pixels,3] uint8 (the views' pixels, flat),
    depth [total_pixels] float32 (mesh_zbuffer's) or None for no occlusion test, cams / dims / offsets as for mesh_zbuffer: contiguous, on the
    device, as they are.  Returns (colors [V,3] float32 in [0,1], views [V] int32: the number of views that counted; zeros where none did).
    No read-back."""
    what = "mesh_photo_colors"
    vp_ = np_ = pp = zp = tables = None
    for on_device in (False, True):
        vp_ = _parts_input(vertices, "vertices", what, torch.float32, cols=3, on_device=on_device)
        V = vertices.shape[0]
        np_ = None if normals is None else _parts_input(normals, "normals", what, torch.float32, cols=3, rows=V, on_device=on_device)
        tables = _photo_views(cams, dims, offsets, total_pixels, z_near, what, on_device)
        total = tables[4]
        pp = _parts_input(photos, "photos", what, torch.uint8, cols=3, rows=total, on_device=on_device)
        zp = None if depth is None else _parts_input(depth, "depth", what, torch.float32, rows=total, on_device=on_device)
        if not on_device:
            depth_tol = float(depth_tol)
            if not (math.isfinite(depth_tol) and depth_tol >= 0.0):
                raise ValueError("crnerf_amd: %s: depth_tol must be finite and >= 0, got %r" % (what, depth_tol))
    cp, dp, op, N, total, z_near = tables
    colors = torch.empty(V, 3, dtype=torch.float32, device=vertices.device)
    views = torch.empty(V, dtype=torch.int32, device=vertices.device)
    if V:
        _lib.check(_lib.load().crnerf_mesh_photo_colors_u8(vp_, np_, V, pp, zp, cp, dp, op, N, total, z_near, depth_tol,
                                                           ctypes.c_void_p(colors.data_ptr()), ctypes.c_void_p(views.data_ptr()),
                                                           _lib.stream_ptr()), "crnerf_mesh_photo_colors_u8")
    return colors, views


def composite(raw, z, noise=None, noise_std=0.0):
    lib = _lib.load()
    raw, z = _f32c(raw, "raw"), _f32c(z, "z")
    R, N = z.shape
    if tuple(raw.shape) != (R, N, 65):
        raise ValueError("composite expects raw [R,N,65], got %s" % (tuple(raw.shape),))
    if noise is not None:
        noise = _f32c(noise, "noise")
    w = torch.empty(R, N, dtype=torch.float32, device=z.device)
    feat = torch.empty(R, 64, dtype=torch.float32, device=z.device)
    depth = torch.empty(R, dtype=torch.float32, device=z.device)
    _lib.check(lib.crnerf_composite_f32(_lib.dev_ptr(raw), _lib.dev_ptr(z), _lib.dev_ptr(noise), float(noise_std), _lib.dev_ptr(w),
                                        _lib.dev_ptr(feat), _lib.dev_ptr(depth), R, N, _lib.stream_ptr()), "crnerf_composite_f32")
    return w, feat, depth


def composite_backward(raw, z, d_feature, d_depth=None, d_weights=None, noise=None, noise_std=0.0):
    lib = _lib.load()
    raw, z, d_feature = _f32c(raw, "raw"), _f32c(z, "z"), _f32c(d_feature, "d_feature")
    R, N = z.shape
    opt = [None if t is None else _f32c(t, n) for t, n in ((d_depth, "d_depth"), (d_weights, "d_weights"), (noise, "noise"))]
    d_raw = torch.empty(R, N, 65, dtype=torch.float32, device=z.device)
    _lib.check(lib.crnerf_composite_backward_f32(_lib.dev_ptr(raw), _lib.dev_ptr(z), _lib.dev_ptr(opt[2]), float(noise_std), _lib.dev_ptr(d_feature),
                                                 _lib.dev_ptr(opt[0]), _lib.dev_ptr(opt[1]), _lib.dev_ptr(d_raw), R, N, _lib.stream_ptr()),
               "crnerf_composite_backward_f32")
    return d_raw


def sample_pdf_merge(z_coarse, weights_coarse, n_importance, u=None, return_samples=False):
    lib = _lib.load()
    z_coarse, weights_coarse = _f32c(z_coarse, "z_coarse"), _f32c(weights_coarse, "weights_coarse")
    R, Nc = z_coarse.shape
    u_stride = 0
    if u is not None:
        u = _f32c(u, "u")
        u_stride = 0 if u.dim() == 1 else n_importance
    zs = torch.empty(R, Nc + n_importance, dtype=torch.float32, device=z_coarse.device)
    smp = torch.empty(R, n_importance, dtype=torch.float32, device=z_coarse.device) if return_samples else None
    _lib.check(lib.crnerf_sample_pdf_merge_f32(_lib.dev_ptr(z_coarse), _lib.dev_ptr(weights_coarse), _lib.dev_ptr(u), u_stride, _lib.dev_ptr(zs),
                                               _lib.dev_ptr(smp), R, Nc, n_importance, _lib.stream_ptr()), "crnerf_sample_pdf_merge_f32")
    return (zs, smp) if return_samples else zs


def _render_args(rays, inputs, noise_std, use_disp, Nc, Ni, out):
    """The crnerf_render_args fields every render entry fills alike: rays, the optional input tensors `inputs` ({field: tensor or None}, made fp32 and
    contiguous), u_stride, noise_std, use_disp, the three counts and the pointer of every output present in `out`.  Returns the struct and the list of
    converted inputs: the struct holds raw pointers, so whoever keeps it keeps that list (and rays, the packs and `out`) alive."""
    keep = [t if t is None else _f32c(t, n) for n, t in inputs.items()]
    a = _lib.RenderArgs()
    a.rays = rays.data_ptr()
    for field, t in zip(inputs, keep):
        setattr(a, field, t.data_ptr() if t is not None else None)
    u = inputs["u"]
    a.u_stride = 0 if (u is None or u.dim() == 1) else Ni
    a.noise_std = float(noise_std)
    a.use_disp = int(bool(use_disp))
    a.n_rays, a.n_samples, a.n_importance = rays.shape[0], Nc, Ni
    for k in ("weights_coarse", "feature_coarse", "depth_coarse", "weights_fine", "feature_fine", "depth_fine", "z_fine"):
        if k in out:
            setattr(a, k, out[k].data_ptr())
    return a, keep


def _resolve_packs(name, packs, repair, what="packs"):
    """(core name, packs, x3 packs of the repair launch or None) of a render under precision `name`; `packs`: a tuple, None where a model is absent.
    "auto" (AutoPacks): the h2 core with the x3 core as its safety net -- render on h2, then the *_f32x3_repair entry re-renders the ray quads that came
    out NaN (a point's activations left fp16's range).  A refused h2 pack (a weight >= 255): the x3 core throughout."""
    if name != "auto":
        return name, packs, repair
    if not isinstance(packs[0], AutoPack) or any(pk is not None and not isinstance(pk, AutoPack) for pk in packs):
        raise ValueError("crnerf_amd: precision='auto' needs %s from pack_mlp_weights(..., precision='auto')" % what)
    x3 = tuple(pk.x3 if pk is not None else None for pk in packs)
    if any(pk is not None and pk.h2 is None for pk in packs):
        return "f32x3", x3, None
    return "f32h2", tuple(pk.h2 if pk is not None else None for pk in packs), x3


def _render(lib, entry, repair_entry, checks, packs, repair, rays, shapes, inputs, noise_std, use_disp, Nc, Ni, extras=None, launcher=False):
    """What every render function does behind its own mode rules: check the packs (`checks`: (core name, pack) pairs) and rays, allocate the output dict
    from `shapes` ((key, shape behind R) pairs), fill the argument block, call `entry` and, with `repair` (x3 packs), `repair_entry` on the same block
    with those packs.  extras(a, out, R, device): the caller's additions to the block and to `out`; returns the arguments of the entry between the block and the
    stream.  launcher=True: (launch, out) -- measurement helper: re-launch the same call on the same buffers with nothing but the C calls on the host."""
    for core_name, pk in checks:
        _check_pack(lib, core_name, pk)
    rays = _f32c(rays, "rays")
    if rays.dim() != 2 or rays.shape[1] != 8:
        raise ValueError("rays must be [R,8], got %s" % (tuple(rays.shape),))
    R, dev = rays.shape[0], rays.device
    out = {k: torch.empty(R, *shape, dtype=torch.float32, device=dev) for k, shape in shapes}      # (sizes as arguments: a tuple parses slower)
    if R == 0:
        return out
    a, keep = _render_args(rays, inputs, noise_std, use_disp, Nc, Ni, out)
    if packs[0] is not None:
        a.packed_coarse = packs[0].data_ptr()
    if packs[1] is not None:
        a.packed_fine = packs[1].data_ptr()
    tail = extras(a, out, R, dev) if extras is not None else ()
    fn, a2 = getattr(lib, entry), _repair_args(a, repair)
    fn2 = getattr(lib, repair_entry) if a2 is not None else None
    # the argument structs hold raw pointers: a launcher that outlives this call keeps EVERY tensor behind them alive (the outputs too: a caller that
    # drops `out` must not hand their memory back to the caching allocator while launch() can still write it)
    held = (keep, rays, packs, out, repair)

    def launch(_held=held):
        _lib.check(fn(ctypes.byref(a), *tail, _lib.stream_ptr()), entry)
        if a2 is not None:        # the ray quads the fp16 range guard poisoned, once more on the scale-free core (a training twin: outputs AND saved state)
            _lib.check(fn2(ctypes.byref(a2), *tail, _lib.stream_ptr()), repair_entry)
    if launcher:
        return launch, out
    launch()
    return out


def render_rays(packed_coarse, packed_fine, rays, n_samples, n_importance, use_disp=False, view_dir=None, z_coarse=None, z_steps=None, u=None,
                noise_coarse=None, noise_fine=None, noise_std=0.0, want_z_fine=False, precision="f32", train=False, launcher=False, rng=None,
                repair_x3=None, lean=False):
    """Fused renderer.  Returns a dict of freshly allocated tensors.  train=True: the training twin
    crnerf_render_rays_train_f32 -- the dict additionally holds what the backward needs: z_coarse (as used), z_fine,
    acts_coarse / acts_fine (crnerf_mlp_forward_train_f32 layout, point = ray * N + sample) and raw_coarse / raw_fine [R,N,65].
    train=True with precision="bf16": crnerf_render_rays_train_bf16, the twin of the opt-in mixed-precision mode (acts_* in the layout
    mlp_backward_mixed(..., fused_acts=True) reads).
    precision="auto": packs from pack_mlp_weights(..., precision="auto"); the h2 core, repaired by the x3 core where it poisoned a ray
    (train=True: crnerf_render_rays_train_f32h2, then crnerf_render_rays_train_f32x3_repair -- saved rows included).
    rng (fp32, f32x3, f32h2, auto): {"seed": int, "ray_offset": int, "perturb": float, "jitter": bool, "u": bool, "noise": bool} -- the stochastic
    steps of rendering.py:125 / :169-176 / :30 drawn INSIDE the kernel (include/crnerf.h CRNERF_RNG_*, csrc/philox.h) instead of
    handed over as tensors; the dict then also holds what was drawn: "z_coarse_used" [R,Nc], and with noise "noise_coarse_used" /
    "noise_fine_used" (standard normal, before noise_std).  rng_fill() returns the same draws as tensors.
    precision="f16": crnerf_render_rays_f16 (packs from pack_mlp_weights(..., precision="f16"); inference only) -- a ray with a point whose operands
    left fp16's range has a NaN feature row.  repair_x3=(coarse x3 pack, fine x3 pack or None): crnerf_render_rays_f32x3_repair re-renders those
    ray quads in the same call, as precision="auto" does behind the h2 core.
    lean=True (precision="f32", "bf16" or "f16"; inference, n_importance > 0): crnerf_render_rays_lean_f32 / _lean_bf16 / _lean_f16 (include/crnerf.h,
    include/crnerf_lean.h) -- the coarse pass stops behind the sigma head and nothing of it reaches HBM; the dict holds feature_fine, depth_fine and
    (want_z_fine) z_fine only, bit-identical to the full call's.  "f16": there is no feature_coarse row to carry the range guard's NaN, so a ray whose
    coarse pass left fp16's range comes back with its whole feature_fine row and its depth_fine NaN (and repair_x3=, which looks for the NaN rows of
    the full call, is refused)."""
    name = resolve(precision)
    repair = None
    if lean:
        if train or rng is not None:
            raise ValueError("crnerf_amd: lean=True is an inference render (no training twin, no in-kernel draws: hand them over as tensors)")
        if name == "auto" or _CORES[name].render_lean is None:
            raise ValueError("crnerf_amd: lean=True exists for precision='f32', 'bf16' and 'f16' (the trunk-only coarse walk is built on the fp32 core "
                             "and on the pair core), got %r" % (name,))
        if int(n_importance) <= 0:
            raise ValueError("crnerf_amd: lean=True needs n_importance > 0 (it returns the fine pass only)")
        if repair_x3 is not None:
            raise ValueError("crnerf_amd: lean=True and repair_x3= are exclusive (the repair re-renders whole rays, coarse outputs included)")
    lib = _lib.load()
    if repair_x3 is not None:
        if name != "f16":
            raise ValueError("crnerf_amd: repair_x3= goes with precision='f16' (precision='auto' brings its own x3 packs)")
        repair = tuple(repair_x3)
    if name == "f16" and (train or rng is not None):
        raise ValueError("crnerf_amd: precision='f16' is an inference mode (no training twin, no in-kernel draws)")
    if launcher and train:
        raise ValueError("crnerf_amd: launcher=True is for the inference entry points")
    name, packs, repair = _resolve_packs(name, (packed_coarse, packed_fine), repair)
    core = _CORES[name]
    Nc, Ni = int(n_samples), int(n_importance)
    if lean:
        shapes = [("feature_fine", (64,)), ("depth_fine", ())]
    elif Ni > 0:
        shapes = [("weights_coarse", (Nc,)), ("feature_coarse", (64,)), ("depth_coarse", ()), ("weights_fine", (Nc + Ni,)), ("feature_fine", (64,)), ("depth_fine", ())]
    else:
        shapes = [("weights_coarse", (Nc,)), ("feature_coarse", (64,)), ("depth_coarse", ())]
    if Ni > 0 and (want_z_fine or train):
        shapes.append(("z_fine", (Nc + Ni,)))

    extras = None
    if train or rng is not None:       # (inference pays for no closure)
        def extras(a, out, R, dev):
            """The in-kernel draws and what they write; train: what the backward needs -- the saved state, handed to the twin behind the block."""
            new = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)  # noqa: E731
            if rng is not None:
                if name == "bf16":
                    raise ValueError("crnerf_amd: in-kernel random draws exist in the fp32 kernels only")
                flags = (_lib.RNG_JITTER if rng.get("jitter") else 0) | (_lib.RNG_U if (rng.get("u") and Ni > 0) else 0) | (_lib.RNG_NOISE if rng.get("noise") else 0)
                a.rng_seed, a.rng_ray_offset, a.rng_flags, a.perturb = int(rng["seed"]) & (2 ** 64 - 1), int(rng.get("ray_offset", 0)), flags, float(rng.get("perturb", 1.0))
                out["z_coarse_used"] = new(R, Nc)
                a.z_coarse_out = out["z_coarse_used"].data_ptr()
                if flags & _lib.RNG_NOISE:
                    out["noise_coarse_used"] = new(R, Nc)
                    a.noise_coarse_out = out["noise_coarse_used"].data_ptr()
                    if Ni > 0:
                        out["noise_fine_used"] = new(R, Nc + Ni)
                        a.noise_fine_out = out["noise_fine_used"].data_ptr()
            if not train:
                return ()
            Nf = Nc + Ni
            acts_bytes = lib.crnerf_mlp_train_mixed_acts_bytes if name == "bf16" else lib.crnerf_mlp_train_acts_bytes
            out["acts_coarse"] = torch.empty(acts_bytes(R * Nc), dtype=torch.uint8, device=dev)
            out["raw_coarse"] = new(R, Nc, 65)
            if Ni > 0:
                out["acts_fine"] = torch.empty(acts_bytes(R * Nf), dtype=torch.uint8, device=dev)
                out["raw_fine"] = new(R, Nf, 65)
            vp = lambda k: ctypes.c_void_p(out[k].data_ptr()) if k in out else None  # noqa: E731
            return vp("acts_coarse"), vp("acts_fine"), vp("raw_coarse"), vp("raw_fine")

    entry, repair_entry = ((core.render_train, "crnerf_render_rays_train_f32x3_repair") if train else
                           (core.render_lean if lean else core.render, "crnerf_render_rays_f32x3_repair"))
    return _render(lib, entry, repair_entry, ((name, packs[0]), (name, packs[1])), packs, repair, rays, shapes,
                   {"view_dir": view_dir, "z_coarse": z_coarse, "z_steps": z_steps, "u": u, "noise_coarse": noise_coarse, "noise_fine": noise_fine},
                   noise_std, use_disp, Nc, Ni, extras, launcher)


def render_coarse_weights(packed_coarse, rays, n_samples, precision="auto", use_disp=False, z_coarse=None, z_steps=None, noise_coarse=None, noise_std=0.0,
                          repair_x3=None):
    """The coarse pass for its compositing weights alone: {"weights_coarse": [R,Nc]}, bit-identical to render_rays(packed_coarse, None, rays, n_samples, 0,
    precision=...)["weights_coarse"] -- every tile stops behind static_sigma, no feature or depth is composited, nothing else is written
    (crnerf_render_coarse_weights_*, include/crnerf_lean_composite.h).  Inference only; random draws come as tensors.
    precision "f32h2" / "f32x3" / "f16": that core, packs as for render_rays.  "f32h2" and "f16" mark a ray that left fp16's range by the word 0x7fc00000
    (a NaN) in weights_coarse[r, 0].  "auto" (an AutoPack): the h2 entry, then crnerf_render_coarse_weights_f32x3_repair, which renders the marked ray
    quads again on the x3 core and leaves at once when there is none; a refused h2 pack: the x3 entry throughout.  "f16" with repair_x3=(the coarse
    model's x3 pack): the same repair behind the fp16 entry."""
    name = resolve(precision)
    if name != "auto" and _CORES[name].coarse_weights is None:
        raise ValueError("crnerf_amd: render_coarse_weights exists for precision='f32h2', 'f32x3', 'auto' and 'f16', got %r" % (name,))
    if repair_x3 is not None and name != "f16":
        raise ValueError("crnerf_amd: repair_x3= goes with precision='f16' (precision='auto' brings its own x3 pack)")
    lib = _lib.load()
    name, packs, repair = _resolve_packs(name, (packed_coarse, None), None if repair_x3 is None else (repair_x3, None), what="a pack")
    return _render(lib, _CORES[name].coarse_weights, "crnerf_render_coarse_weights_f32x3_repair", [(name, packs[0]), ("f32x3", repair[0] if repair else None)],
                   packs, repair, rays, [("weights_coarse", (int(n_samples),))],
                   {"view_dir": None, "z_coarse": z_coarse, "z_steps": z_steps, "u": None, "noise_coarse": noise_coarse, "noise_fine": None},
                   noise_std, use_disp, int(n_samples), 0)


_LEAN_X = {"f32x3": "crnerf_render_rays_lean_f32x3", "f32h2": "crnerf_render_rays_lean_f32h2"}      # include/crnerf_lean_x.h


def render_rays_lean_x(packed_coarse, packed_fine, rays, n_samples, n_importance, precision="auto", use_disp=False, view_dir=None, z_coarse=None,
                       z_steps=None, u=None, noise_coarse=None, noise_fine=None, noise_std=0.0, want_z_fine=False, launcher=False):
    """The lean render on the fp32-accurate split cores (crnerf_render_rays_lean_f32x3 / _f32h2 / _f32x3_repair, include/crnerf_lean_x.h):
    {"feature_fine", "depth_fine"[, "z_fine"]}, bit-identical to render_rays(..., precision=...)'s -- the coarse tiles stop behind static_sigma, no
    coarse feature or depth is composited, and nothing else is allocated or written.  Inference only; random draws come as tensors.
    precision "f32x3" / "f32h2": that core, packs as for render_rays.  "f32h2" has no feature_coarse row to carry the range guard's NaN: a ray whose
    coarse trunk walk left fp16's range comes back with its whole feature_fine row and its depth_fine NaN.  "auto" (AutoPacks): the h2 entry, then
    crnerf_render_rays_lean_f32x3_repair on the same block, which renders the ray quads with a NaN feature_fine[r, 0] again, lean, on the x3 core
    and leaves at once where there is none; a refused h2 pack: the x3 entry throughout."""
    name = resolve(precision)
    if name != "auto" and name not in _LEAN_X:
        raise ValueError("crnerf_amd: render_rays_lean_x exists for precision='f32x3', 'f32h2' and 'auto' (render_rays(..., lean=True) has the "
                         "others), got %r" % (name,))
    Nc, Ni = int(n_samples), int(n_importance)
    if Ni <= 0:
        raise ValueError("crnerf_amd: render_rays_lean_x needs n_importance > 0 (it returns the fine pass only)")
    if not 3 <= Nc <= 256 or Ni > 256:
        raise ValueError("crnerf_amd: render_rays_lean_x is the fused kernel's: n_samples in [3, 256] and n_importance in [1, 256], got %d + %d" % (Nc, Ni))
    if packed_coarse is None or packed_fine is None:
        raise ValueError("crnerf_amd: render_rays_lean_x needs both models' packs")
    name, packs, repair = _resolve_packs(name, (packed_coarse, packed_fine), None)
    lib = _lib.load()
    shapes = [("feature_fine", (64,)), ("depth_fine", ())] + ([("z_fine", (Nc + Ni,))] if want_z_fine else [])
    checks = [(name, packs[0]), (name, packs[1])] + ([("f32x3", repair[0]), ("f32x3", repair[1])] if repair else [])
    return _render(lib, _LEAN_X[name], "crnerf_render_rays_lean_f32x3_repair", checks, packs, repair, rays, shapes,
                   {"view_dir": view_dir, "z_coarse": z_coarse, "z_steps": z_steps, "u": u, "noise_coarse": noise_coarse, "noise_fine": noise_fine},
                   noise_std, use_disp, Nc, Ni, None, launcher)


def render_rays_bf16_fine(packed_fine_bf16, rays, weights_coarse, n_samples, n_importance, use_disp=False, view_dir=None, z_coarse=None, z_steps=None, u=None,
                          noise_fine=None, noise_std=0.0, want_z_fine=False, lean=False):
    """crnerf_render_rays_bf16_fine: sample_pdf + z merge on `weights_coarse` [R,Nc] (rendered by another core, e.g. render_rays(..., n_importance=0,
    precision="auto")) and the fine model on the bf16 matrix cores, fused -- {"weights_fine", "feature_fine", "depth_fine"[, "z_fine"]}.
    lean=True: crnerf_render_rays_lean_bf16_fine -- the same launch without weights_fine (neither allocated nor written); the other tensors are
    bit-identical."""
    lib = _lib.load()
    _check_pack(lib, "bf16", packed_fine_bf16)
    rays, weights_coarse = _f32c(rays, "rays"), _f32c(weights_coarse, "weights_coarse")
    Nc, Ni = int(n_samples), int(n_importance)
    if rays.dim() != 2 or rays.shape[1] != 8 or tuple(weights_coarse.shape) != (rays.shape[0], Nc) or Ni <= 0:
        raise ValueError("render_rays_bf16_fine: rays [R,8], weights_coarse [R,%d] and n_importance > 0 expected, got %s / %s / %d"
                         % (Nc, tuple(rays.shape), tuple(weights_coarse.shape), Ni))
    shapes = ([] if lean else [("weights_fine", (Nc + Ni,))]) + [("feature_fine", (64,)), ("depth_fine", ())] + ([("z_fine", (Nc + Ni,))] if want_z_fine else [])
    # weights_coarse is an INPUT of this entry point
    return _render(lib, "crnerf_render_rays_lean_bf16_fine" if lean else "crnerf_render_rays_bf16_fine", None, (), (None, packed_fine_bf16), None, rays, shapes,
                   {"view_dir": view_dir, "z_coarse": z_coarse, "z_steps": z_steps, "u": u, "noise_fine": noise_fine, "weights_coarse": weights_coarse},
                   noise_std, use_disp, Nc, Ni)


def _repair_args(a, repair):
    """The argument block of the h2 render with the x3 packs in place of the h2 ones (crnerf_render_rays_f32x3_repair)."""
    if repair is None:
        return None
    a2 = _lib.RenderArgs()
    ctypes.memmove(ctypes.byref(a2), ctypes.byref(a), ctypes.sizeof(a))
    a2.packed_coarse = repair[0].data_ptr()
    a2.packed_fine = repair[1].data_ptr() if repair[1] is not None else None
    return a2


_IN_KERNEL_RNG = [None]


def set_in_kernel_rng(on=True):
    """True (default): grad-mode renders through the fused fp32 kernel draw their stratified jitter / sample_pdf uniforms / density
    noise inside the kernel (Philox keyed on (seed, ray, sample)); False: torch.rand / torch.randn tensors handed to the kernel, the
    round-1/2 path.  CRNERF_IN_KERNEL_RNG=0 does the same from the environment."""
    _IN_KERNEL_RNG[0] = bool(on)


def in_kernel_rng():
    import os
    if _IN_KERNEL_RNG[0] is not None:
        return _IN_KERNEL_RNG[0]
    return os.environ.get("CRNERF_IN_KERNEL_RNG", "1") not in ("0", "")


def rng_fill(n_rays, n, seed, stream, ray_offset=0, device="cuda"):
    """The renderer's in-kernel draws as a tensor [n_rays, n] (crnerf_rng_fill_f32): stream 0 = jitter uniforms, 1 = sample_pdf
    uniforms, 2 = coarse noise, 3 = fine noise.  Feeding these through render_rays' tensor arguments reproduces the in-kernel
    path bit for bit (tests/test_gpu_rng.py)."""
    lib = _lib.load()
    out = torch.empty(int(n_rays), int(n), dtype=torch.float32, device=device)
    _lib.check(lib.crnerf_rng_fill_f32(ctypes.c_void_p(out.data_ptr()), int(n_rays), int(n), int(seed) & (2 ** 64 - 1), int(stream), int(ray_offset),
                                       _lib.stream_ptr()), "crnerf_rng_fill_f32")
    return out


# ---------------------------------------------------------------- cross-ray decoder pieces
_ws_cache = {}


def crossray_workspace(device):
    # one per device AND stream: pipeline.TrainingSystem runs independent decodes side by side on their own streams (round 6)
    key = (device.type, device.index, int(_lib.stream_ptr().value or 0))
    ws = _ws_cache.get(key)
    if ws is None:
        ws = torch.empty(_lib.load().crnerf_crossray_workspace_bytes(), dtype=torch.uint8, device=device)
        _ws_cache[key] = ws
    return ws


def crossray_chansum(x):
    lib = _lib.load()
    x = _f32c(x, "x")
    out = torch.empty(64, dtype=torch.float32, device=x.device)
    ws = crossray_workspace(x.device)
    _lib.check(lib.crnerf_crossray_chansum_f32(_lib.dev_ptr(x), x.shape[0], _lib.dev_ptr(out), ctypes.c_void_p(ws.data_ptr()),
                                               _lib.stream_ptr()), "crnerf_crossray_chansum_f32")
    return out


def crossray_gram(x, mean, cnn):
    lib = _lib.load()
    x, mean = _f32c(x, "x"), _f32c(mean, "mean")
    cnn = [_f32c(t.detach(), "cnn") for t in cnn]
    out = torch.empty(1024, dtype=torch.float32, device=x.device)
    ws = crossray_workspace(x.device)
    _lib.check(lib.crnerf_crossray_gram_f32(_lib.dev_ptr(x), x.shape[0], _lib.dev_ptr(mean), _lib.ptr_array(cnn, "cnn"), _lib.dev_ptr(out),
                                            ctypes.c_void_p(ws.data_ptr()), _lib.stream_ptr()), "crnerf_crossray_gram_f32")
    return out


def crossray_matrix(gram_sum, count, fc_w, fc_b):
    lib = _lib.load()
    fc_w, fc_b = _f32c(fc_w.detach(), "fc_w"), _f32c(fc_b.detach(), "fc_b")
    out = torch.empty(1024, dtype=torch.float32, device=gram_sum.device)
    _lib.check(lib.crnerf_crossray_matrix_f32(_lib.dev_ptr(gram_sum), float(count), _lib.dev_ptr(fc_w), _lib.dev_ptr(fc_b),
                                              _lib.dev_ptr(out), _lib.stream_ptr()), "crnerf_crossray_matrix_f32")
    return out


def crossray_fold(s_matrix, c_matrix, c_mean, s_mean, lin):
    lib = _lib.load()
    lin = [_f32c(t.detach(), "lin") for t in lin]
    out = torch.empty(195, dtype=torch.float32, device=lin[0].device)
    _lib.check(lib.crnerf_crossray_fold_f32(_lib.dev_ptr(s_matrix), _lib.dev_ptr(c_matrix), _lib.dev_ptr(c_mean), _lib.dev_ptr(s_mean),
                                            _lib.ptr_array(lin, "lin"), _lib.dev_ptr(out), _lib.stream_ptr()), "crnerf_crossray_fold_f32")
    return out


def _planar_out(out, HW, like):
    """The planar rgb destination [3,HW] of a decode: a fresh tensor, or the caller's -- which may be a view with a plane stride of its own
    (the ABI's plane_stride), each plane dense."""
    if out is None:
        return torch.empty(3, HW, dtype=torch.float32, device=like.device)
    if tuple(out.shape) != (3, HW) or out.dtype != torch.float32 or out.device != like.device or (HW > 1 and out.stride(1) != 1) or out.stride(0) < HW:
        raise ValueError("crnerf_amd: out must be a float32 [3,%d] tensor on %s with dense planes, got %s %s strides %s on %s"
                         % (HW, like.device, out.dtype, tuple(out.shape), out.stride(), out.device))
    return out


def crossray_apply(x, affine, out=None):
    lib = _lib.load()
    x = _f32c(x, "x")
    HW = x.shape[0]
    out = _planar_out(out, HW, x)
    _lib.check(lib.crnerf_crossray_apply_f32(_lib.dev_ptr(x), HW, _lib.dev_ptr(affine), ctypes.c_void_p(out.data_ptr()), out.stride(0), _lib.stream_ptr()),
               "crnerf_crossray_apply_f32")
    return out


def crossray_decode(content_pm, style_pm, weights, out=None):
    """Whole style_net.forward from one host call.  content_pm [HW,64], style_pm [HWs,64] or None,
    weights: the 22 parameter tensors in state_dict order.  Returns planar rgb [3,HW]."""
    lib = _lib.load()
    x = _f32c(content_pm, "content")
    s = _f32c(style_pm, "style") if style_pm is not None else None
    ws = crossray_workspace(x.device)
    HW = x.shape[0]
    out = _planar_out(out, HW, x)
    arr = _lib.ptr_array(_wlist(weights, "decoder weight"), "decoder weight")
    _lib.check(lib.crnerf_crossray_decode_f32(_lib.dev_ptr(x), HW, _lib.dev_ptr(s), s.shape[0] if s is not None else 0, arr,
                                              ctypes.c_void_p(ws.data_ptr()), ctypes.c_void_p(out.data_ptr()), out.stride(0), _lib.stream_ptr()),
               "crnerf_crossray_decode_f32")
    return out


# ---- appearance sweep (include/crnerf_sweep.h): the styles' statistics once, then one content grid decoded under all of them
_COOP_MAX_PIXELS = 4096      # GRAM_COOP_MAX_PIXELS (csrc/crossray.hip): where the single decode switches its Gram reduction


def _sweep_small_path(content_hw, style_hw):
    """The single decode sums its partial Grams in one launch only when BOTH grids have <= 4096 pixels; the order of the sum follows."""
    return content_hw <= _COOP_MAX_PIXELS and style_hw <= _COOP_MAX_PIXELS


class StyleStats:
    """What a style contributes to a decode, for S styles: `stats` [S,1088] float32 on the device (channel mean, then the 32 x 32 style matrix),
    `S`, `style_hw` (pixels of each style grid) and `small_path` -- the side of the single decode's reduction switch the stats were made for."""
    __slots__ = ("stats", "S", "style_hw", "small_path")

    def __init__(self, stats, style_hw, small_path):
        self.stats, self.S, self.style_hw, self.small_path = stats, int(stats.shape[0]), int(style_hw), bool(small_path)


def _sweep_inference_only(weights, what):
    if torch.is_grad_enabled() and any(getattr(t, "requires_grad", False) for t in weights):
        raise ValueError("crnerf_amd: %s is an inference call (no backward): run it under torch.no_grad() or with frozen weights" % what)


def _sweep_grid(t, name):
    if not isinstance(t, torch.Tensor) or t.dim() != 2 or t.shape[1] != 64:
        raise ValueError("crnerf_amd: %s must be a pixel-major [HW,64] grid, got %s" % (name, tuple(t.shape) if isinstance(t, torch.Tensor) else type(t).__name__))
    return t


def _sweep_on_gpu(tensors, name):
    for t in tensors:
        if not t.is_cuda:
            raise ValueError("crnerf_amd: %s must be a GPU tensor (the HIP path has no CPU fallback), got one on %s" % (name, t.device))


def crossray_style_stats(style_pms, weights, content_hw):
    """The style half of crossray_decode for S style grids, once per sweep.  style_pms: S tensors [HWs,64] of one size (or one [S,HWs,64]);
    weights: the 22 decoder tensors; content_hw: the pixel count of the content grids the stats will be used with (it decides the summation
    order, as in the single decode).  Returns a StyleStats."""
    grids = list(style_pms.unbind(0)) if isinstance(style_pms, torch.Tensor) and style_pms.dim() == 3 else list(style_pms)
    if not grids:
        raise ValueError("crnerf_amd: crossray_style_stats needs at least one style grid")
    for g in grids:
        _sweep_grid(g, "style grid")
    hws = int(grids[0].shape[0])
    if hws < 1 or any(int(g.shape[0]) != hws for g in grids):
        raise ValueError("crnerf_amd: the style grids of a sweep must share one size >= 1, got %s" % ([int(g.shape[0]) for g in grids],))
    content_hw = int(content_hw)
    if content_hw < 1:
        raise ValueError("crnerf_amd: content_hw must be the pixel count of the content grids (>= 1), got %d" % content_hw)
    weights = list(weights)
    if len(weights) != 22:
        raise ValueError("crnerf_amd: expected the 22 decoder tensors, got %d" % len(weights))
    _sweep_inference_only(weights, "crossray_style_stats")
    _sweep_on_gpu(grids, "a style grid")
    lib = _lib.load()
    styles = _f32c(torch.stack([g.detach() for g in grids], 0), "style grids")
    S = styles.shape[0]
    stats = torch.empty(S, _lib.SWEEP_STATS_FLOATS, dtype=torch.float32, device=styles.device)
    ws = crossray_workspace(styles.device)
    arr = _lib.ptr_array(_wlist(weights, "decoder weight"), "decoder weight")
    for s0 in range(0, S, _lib.SWEEP_MAX_STYLES):
        n = min(_lib.SWEEP_MAX_STYLES, S - s0)
        _lib.check(lib.crnerf_crossray_style_stats_f32(ctypes.c_void_p(styles[s0].data_ptr()), n, hws, content_hw, arr, ctypes.c_void_p(ws.data_ptr()),
                                                       ctypes.c_void_p(stats[s0].data_ptr()), _lib.stream_ptr()), "crnerf_crossray_style_stats_f32")
    return StyleStats(stats, hws, _sweep_small_path(content_hw, hws))


def _sweep_out(out, S, HW, u8, like):
    """The destination of a multi decode: [S,3,HW] float32 planes or [S,HW,3] uint8 frames, fresh or the caller's -- which may be a view whose
    images (and, for float, planes) are padded.  Returns (tensor, style_stride, plane_stride) in elements."""
    shape, dtype = ((S, HW, 3), torch.uint8) if u8 else ((S, 3, HW), torch.float32)
    if out is None:
        out = torch.empty(shape, dtype=dtype, device=like.device)
    elif not isinstance(out, torch.Tensor) or tuple(out.shape) != shape or out.dtype != dtype or out.device != like.device:
        raise ValueError("crnerf_amd: out must be a %s %s tensor on %s" % (dtype, shape, like.device))
    if u8:
        image, plane = 3 * HW, 0
        dense = out.stride(2) == 1 and (HW <= 1 or out.stride(1) == 3)
    else:
        plane = out.stride(1)
        image = 2 * plane + HW
        dense = (HW <= 1 or out.stride(2) == 1) and plane >= HW
    if not dense or (S > 1 and out.stride(0) < image):
        raise ValueError("crnerf_amd: out %s with strides %s: every image must be dense (padding only between images%s)"
                         % (shape, out.stride(), "" if u8 else " and planes"))
    return out, (out.stride(0) if S > 1 else image), plane


def crossray_decode_multi(content_pm, stats, weights, out=None, u8=False):
    """One content grid [HW,64] decoded under the S styles of `stats` (crossray_style_stats): the content's sums and Gram once, S folds, one apply
    pass over the grid.  Returns [S,3,HW] float32 -- image s bit-identical to crossray_decode(content_pm, style_s, weights) -- or, u8=True,
    [S,HW,3] uint8 frames (clamp(v, 0, 1) * 255, truncated; NaN -> 0).  More than 16 styles are split into several calls."""
    _sweep_grid(content_pm, "content")
    if not isinstance(stats, StyleStats):
        raise ValueError("crnerf_amd: stats must come from crossray_style_stats, got %s" % type(stats).__name__)
    HW = int(content_pm.shape[0])
    if HW > 0 and stats.small_path != _sweep_small_path(HW, stats.style_hw):
        raise ValueError("crnerf_amd: these stats were made for content grids %s %d pixels and cannot be used with one of %d: the decode sums in "
                         "another order there; rebuild them with crossray_style_stats(..., content_hw=%d)"
                         % ("of at most" if stats.small_path else "beyond", _COOP_MAX_PIXELS, HW, HW))
    weights = list(weights)
    if len(weights) != 22:
        raise ValueError("crnerf_amd: expected the 22 decoder tensors, got %d" % len(weights))
    _sweep_inference_only(weights, "crossray_decode_multi")
    _sweep_on_gpu([content_pm, stats.stats], "content / stats")
    if stats.stats.device != content_pm.device:
        raise ValueError("crnerf_amd: content is on %s, the stats on %s" % (content_pm.device, stats.stats.device))
    S = stats.S
    out, style_stride, plane_stride = _sweep_out(out, S, HW, u8, content_pm)
    lib = _lib.load()
    x = _f32c(content_pm.detach(), "content")
    ws = crossray_workspace(x.device)
    arr = _lib.ptr_array(_wlist(weights, "decoder weight"), "decoder weight")
    a = _lib.SweepDecodeArgs()
    a.content, a.HW, a.style_HW = x.data_ptr(), HW, stats.style_hw
    a.out_kind = _lib.SWEEP_OUT_U8 if u8 else _lib.SWEEP_OUT_F32
    a.weights, a.workspace = ctypes.cast(arr, ctypes.POINTER(ctypes.c_void_p)), ws.data_ptr()
    a.style_stride, a.plane_stride = style_stride, plane_stride
    for s0 in range(0, S, _lib.SWEEP_MAX_STYLES):
        a.S = min(_lib.SWEEP_MAX_STYLES, S - s0)
        a.stats, a.out = stats.stats[s0].data_ptr(), out[s0].data_ptr()
        _lib.check(lib.crnerf_crossray_decode_multi_f32(ctypes.byref(a), _lib.stream_ptr()), "crnerf_crossray_decode_multi_f32")
    return out


def encoder_forward(image, weights):
    """encoder_sameoutputsize.forward: image [1,3,H,W] or [3,H,W] -> pixel-major style grid [1024,64]."""
    lib = _lib.load()
    img = _f32c(image.reshape(3, image.shape[-2], image.shape[-1]), "image")
    H, W = img.shape[-2], img.shape[-1]
    ws = torch.empty(lib.crnerf_encoder_workspace_bytes(H, W), dtype=torch.uint8, device=img.device)
    out = torch.empty(1024, 64, dtype=torch.float32, device=img.device)
    arr = _lib.ptr_array(_wlist(weights, "encoder weight"), "encoder weight")
    _lib.check(lib.crnerf_encoder_forward_f32(_lib.dev_ptr(img), H, W, arr, ctypes.c_void_p(ws.data_ptr()), _lib.dev_ptr(out), _lib.stream_ptr()),
               "crnerf_encoder_forward_f32")
    return out


def decoder_content_backward(content_pm, rgb_w, rgb, d_rgb):
    """Backward of the decoder-only ('content') call: returns (d_content[HW,64], d_w[3,64], d_b[3])."""
    lib = _lib.load()
    x, w = _f32c(content_pm, "content"), _f32c(rgb_w.detach(), "rgb_w").reshape(3, 64)
    rgb, d_rgb = _f32c(rgb, "rgb"), _f32c(d_rgb, "d_rgb")
    HW = x.shape[0]
    dx, dw, db = torch.empty_like(x), torch.empty(3, 64, device=x.device), torch.empty(3, device=x.device)
    work = torch.empty(lib.crnerf_decoder_content_backward_workspace_bytes(HW), dtype=torch.uint8, device=x.device)
    _lib.check(lib.crnerf_decoder_content_backward_f32(_lib.dev_ptr(x), HW, _lib.dev_ptr(w), _lib.dev_ptr(rgb), rgb.stride(0), _lib.dev_ptr(d_rgb),
                                                       d_rgb.stride(0), ctypes.c_void_p(work.data_ptr()), _lib.dev_ptr(dx), _lib.dev_ptr(dw),
                                                       _lib.dev_ptr(db), _lib.stream_ptr()), "crnerf_decoder_content_backward_f32")
    return dx, dw, db


def encoder_forward_train(image, weights):
    """Forward of the appearance encoder that keeps the layer outputs: returns (grid [1024,64], saved, (H, W))."""
    lib = _lib.load()
    img = _f32c(image, "image")
    if img.dim() == 4:
        img = img[0]
    _, H, W = img.shape
    ws = _wlist(weights, "encoder weight")
    saved = torch.empty(lib.crnerf_encoder_train_saved_bytes(H, W), dtype=torch.uint8, device=img.device)
    out = torch.empty(1024, 64, dtype=torch.float32, device=img.device)
    _lib.check(lib.crnerf_encoder_forward_train_f32(_lib.dev_ptr(img), H, W, _lib.ptr_array(ws, "encoder weight"), ctypes.c_void_p(saved.data_ptr()),
                                                    _lib.dev_ptr(out), _lib.stream_ptr()), "crnerf_encoder_forward_train_f32")
    return out, saved, (H, W)


def encoder_backward(weights, saved, hw, out, d_out, want_d_image=True):
    lib = _lib.load()
    H, W = hw
    ws = _wlist(weights, "encoder weight")
    grads = [torch.empty_like(t) for t in ws]
    d_img = torch.empty(3, H, W, dtype=torch.float32, device=out.device) if want_d_image else None
    scratch = torch.empty(lib.crnerf_encoder_train_scratch_bytes(H, W), dtype=torch.uint8, device=out.device)
    _lib.check(lib.crnerf_encoder_backward_f32(H, W, _lib.ptr_array(ws, "encoder weight"), ctypes.c_void_p(saved.data_ptr()), _lib.dev_ptr(out),
                                               _lib.dev_ptr(_f32c(d_out, "d_out")), ctypes.c_void_p(scratch.data_ptr()),
                                               _lib.ptr_array(grads, "encoder grad"), _lib.dev_ptr(d_img), _lib.stream_ptr()),
               "crnerf_encoder_backward_f32")
    return grads, d_img


def encoder_forward_train_band(image_rows, h_image, row0, o0, o1, weights):
    """crnerf_encoder_forward_train_band_f32: the training forward of the appearance encoder over rows [row0, row0 + H) of an image of `h_image` rows
    (image_rows [3,H,W] contiguous) -> (rows [o0, o1) of the 32 x 32 grid as [(o1 - o0) * 32, 64], saved, (H, W))."""
    lib = _lib.load()
    img = _f32c(image_rows, "image_rows")
    _, H, W = img.shape
    ws = _wlist(weights, "encoder weight")
    saved = torch.empty(lib.crnerf_encoder_train_band_saved_bytes(H, W, o1 - o0), dtype=torch.uint8, device=img.device)
    out = torch.empty((o1 - o0) * 32, 64, dtype=torch.float32, device=img.device)
    _lib.check(lib.crnerf_encoder_forward_train_band_f32(_lib.dev_ptr(img), H, W, int(h_image), int(row0), int(o0), int(o1), _lib.ptr_array(ws, "encoder weight"),
                                                         ctypes.c_void_p(saved.data_ptr()), _lib.dev_ptr(out), _lib.stream_ptr()), "crnerf_encoder_forward_train_band_f32")
    return out, saved, (H, W)


def encoder_backward_band(weights, saved, hw, h_image, row0, o0, o1, out, d_out, want_d_image=True):
    """crnerf_encoder_backward_band_f32 -> (this band's part of the 14 weight gradients, d_image_rows [3,H,W] or None)."""
    lib = _lib.load()
    H, W = hw
    ws = _wlist(weights, "encoder weight")
    grads = [torch.empty_like(t) for t in ws]
    d_img = torch.empty(3, H, W, dtype=torch.float32, device=out.device) if want_d_image else None
    scratch = torch.empty(lib.crnerf_encoder_train_band_scratch_bytes(H, W, o1 - o0), dtype=torch.uint8, device=out.device)
    _lib.check(lib.crnerf_encoder_backward_band_f32(H, W, int(h_image), int(row0), int(o0), int(o1), _lib.ptr_array(ws, "encoder weight"),
                                                    ctypes.c_void_p(saved.data_ptr()), _lib.dev_ptr(out), _lib.dev_ptr(_f32c(d_out, "d_out")),
                                                    ctypes.c_void_p(scratch.data_ptr()), _lib.ptr_array(grads, "encoder grad"), _lib.dev_ptr(d_img), _lib.stream_ptr()),
               "crnerf_encoder_backward_band_f32")
    return grads, d_img


def crossray_decode_backward(content_pm, style_pm, weights, d_rgb):
    """Backward of crossray_decode: returns (d_content[HW,64], d_style[HWs,64], [22 weight gradients])."""
    lib = _lib.load()
    x, s, d_rgb = _f32c(content_pm, "content"), _f32c(style_pm, "style"), _f32c(d_rgb, "d_rgb")
    HW, HWs = x.shape[0], s.shape[0]
    ws_t = _wlist(weights, "decoder weight")
    grads = [torch.empty_like(t) for t in ws_t]
    dx, ds = torch.empty_like(x), torch.empty_like(s)
    work = torch.empty(lib.crnerf_crossray_backward_workspace_bytes(HW, HWs), dtype=torch.uint8, device=x.device)
    _lib.check(lib.crnerf_crossray_decode_backward_f32(_lib.dev_ptr(x), HW, _lib.dev_ptr(s), HWs, _lib.ptr_array(ws_t, "decoder weight"),
                                                       _lib.dev_ptr(d_rgb), d_rgb.stride(0), ctypes.c_void_p(work.data_ptr()), _lib.dev_ptr(dx),
                                                       _lib.dev_ptr(ds), _lib.ptr_array(grads, "decoder grad"), _lib.stream_ptr()),
               "crnerf_crossray_decode_backward_f32")
    return dx, ds, grads


def crossray_decode_sharded(content_pm, style_pm, weights, phase, xchg, count_global, rgb=None):
    """One phase (0, 1, 2) of the ray-sharded decode; the caller all-reduces xchg[0:64] after phase 0 and
    xchg[64:1088] after phase 1.  Returns rgb [3, HW_local] after phase 2."""
    lib = _lib.load()
    s = _f32c(style_pm, "style")
    n = content_pm.shape[0]
    x = _f32c(content_pm, "content") if n else None
    ws = crossray_workspace(s.device)
    arr = _lib.ptr_array(_wlist(weights, "decoder weight"), "decoder weight")
    if phase == 2 and rgb is None:
        rgb = torch.empty(3, n, dtype=torch.float32, device=s.device)
    _lib.check(lib.crnerf_crossray_decode_sharded_f32(_lib.dev_ptr(x), n, _lib.dev_ptr(s), s.shape[0], arr, int(phase), _lib.dev_ptr(xchg),
                                                      float(count_global), ctypes.c_void_p(ws.data_ptr()),
                                                      _lib.dev_ptr(rgb) if (rgb is not None and n) else None,
                                                      rgb.stride(0) if (rgb is not None and n) else 0, _lib.stream_ptr()),
               "crnerf_crossray_decode_sharded_f32")
    return rgb


def crossray_decode_backward_sharded(content_pm, style_pm, weights, d_rgb_local, phase, fwd_xchg, count_global, xb, state=None):
    """One phase (0, 1, 2) of the ray-sharded decoder backward (crnerf_crossray_decode_backward_sharded_f32).  state: None for phase 0 -- the call
    allocates (workspace, d_content, d_style, grads) and returns it; pass it back for phases 1 and 2.  The caller all-reduces xb[0:320] after
    phase 0 and xb[320:384] after phase 1.  After phase 2: d_content [HW_local,64], d_style [HWs,64], grads (22; [8..13] are this rank's part)."""
    lib = _lib.load()
    x, s, d_rgb = _f32c(content_pm, "content"), _f32c(style_pm, "style"), _f32c(d_rgb_local, "d_rgb")
    HW, HWs = x.shape[0], s.shape[0]
    ws_t = _wlist(weights, "decoder weight")
    if state is None:
        state = (torch.empty(lib.crnerf_crossray_backward_workspace_bytes(HW, HWs), dtype=torch.uint8, device=x.device), torch.empty_like(x),
                 torch.empty_like(s), [torch.empty_like(t) for t in ws_t])
    work, dx, ds, grads = state
    _lib.check(lib.crnerf_crossray_decode_backward_sharded_f32(_lib.dev_ptr(x), HW, _lib.dev_ptr(s), HWs, _lib.ptr_array(ws_t, "decoder weight"),
                                                               _lib.dev_ptr(d_rgb), d_rgb.stride(0), ctypes.c_void_p(work.data_ptr()), _lib.dev_ptr(dx),
                                                               _lib.dev_ptr(ds), _lib.ptr_array(grads, "decoder grad"), int(phase), _lib.dev_ptr(fwd_xchg),
                                                               float(count_global), _lib.dev_ptr(xb), _lib.stream_ptr()),
               "crnerf_crossray_decode_backward_sharded_f32")
    return state


# ---------------------------------------------------------------- training-side neighbours
LOSS_KEYS = ("kl_a", "rec_a_random", "c_l", "content_constraint", "r_ms", "r_md", "f_l")


def _rgb2d(t, name):
    if t.dim() != 2 or t.shape[1] != 3:
        raise ValueError("crnerf_amd: %s must be [R,3], got %s" % (name, tuple(t.shape)))
    if not t.is_cuda:
        raise RuntimeError("crnerf_amd: %s is on %s; the HIP path needs GPU tensors and has no CPU fallback" % (name, t.device))
    if t.dtype != torch.float32:
        raise TypeError("crnerf_amd: %s must be float32" % name)
    return t


def _dense_flat(t):
    """1-D view of t's elements in MEMORY order when t is a permutation of a contiguous tensor (non-overlapping, no gaps), else None."""
    if t.is_contiguous():
        return t.reshape(-1)
    expect = 1
    for d in sorted(range(t.dim()), key=lambda d: t.stride(d)):
        if t.shape[d] == 1:
            continue
        if t.stride(d) != expect:
            return None
        expect *= t.shape[d]
    return t.as_strided((t.numel(),), (1,))


def loss_args(rgb_coarse, targets, rgb_fine=None, mask=None, a_embedded=None, a_embedded_random=None, a_embedded_random_rec=None,
              content_wo=None, content_with=None, mse_on_appearance=False, coef=1.0, weight_kl=0.0, weight_rec_a=0.0,
              weight_content=0.0, mask_size_weight=0.0, mask_digit_weight=0.0):
    """Fill struct crnerf_loss_args.  rgb tensors may be any strided [R,3] view (e.g. the decoder's planar output
    rearranged the reference's way); everything else is made contiguous.  Returns (struct, keep-alive list)."""
    a = _lib.LossArgs()
    keep = []
    R = rgb_coarse.shape[0]
    for name, t in (("rgb_coarse", rgb_coarse), ("rgb_fine", rgb_fine), ("targets", targets)):
        if t is None:
            setattr(a, name, None)
            continue
        t = _rgb2d(t.detach(), name)
        if t.shape[0] != R:
            raise ValueError("crnerf_amd: %s has %d rows, rgb_coarse %d" % (name, t.shape[0], R))
        keep.append(t)
        setattr(a, name, t.data_ptr())
        setattr(a, name + "_row_stride", t.stride(0))
        setattr(a, name + "_chan_stride", t.stride(1))
    flat = lambda t, n: None if t is None else _f32c(t.detach(), n).reshape(-1)  # noqa: E731
    # The embedding / content terms are full reductions over one tensor or over a same-shaped pair: the element ORDER does not matter as long
    # as both members of a pair are walked in the same one.  The encoders' outputs are NCHW *views* of pixel-major memory; read in memory order
    # they need no transposing copy here (and their gradients, written in the same order, none in the encoder's backward).
    def memory_order(*ts):
        if any(t is None for t in ts):
            return None
        ts = [t.detach() for t in ts]
        if any(t.dtype != torch.float32 or not t.is_cuda or t.shape != ts[0].shape or t.stride() != ts[0].stride() for t in ts):
            return None
        views = [_dense_flat(t) for t in ts]
        return None if any(v is None for v in views) else views
    layouts = {}
    m = flat(mask, "out_mask")
    got = memory_order(a_embedded)
    ae = got[0] if got else flat(a_embedded, "a_embedded")
    if got and not a_embedded.is_contiguous():
        layouts["a_embedded"] = a_embedded.stride()
    got = memory_order(a_embedded_random, a_embedded_random_rec)
    ar, arr = got if got else (flat(a_embedded_random, "a_embedded_random"), flat(a_embedded_random_rec, "a_embedded_random_rec"))
    if got and not a_embedded_random_rec.is_contiguous():
        layouts["a_embedded_random_rec"] = a_embedded_random_rec.stride()
    got = memory_order(content_wo, content_with)
    cw, cwi = got if got else (flat(content_wo, "content_wo_a_embed"), flat(content_with, "content_with_a_embed"))
    if got and not content_wo.is_contiguous():
        layouts["content_wo_a_embed"] = layouts["content_with_a_embed"] = content_wo.stride()
    if m is not None and m.numel() != R:
        raise ValueError("crnerf_amd: out_mask must have one value per ray")
    if arr is not None and (ar is None or ar.numel() != arr.numel()):
        raise ValueError("crnerf_amd: a_embedded_random and a_embedded_random_rec must have the same size")
    if (cw is None) != (cwi is None) or (cw is not None and cw.numel() != cwi.numel()):
        raise ValueError("crnerf_amd: content_wo_a_embed and content_with_a_embed come as a same-sized pair")
    keep += [t for t in (m, ae, ar, arr, cw, cwi) if t is not None]
    p = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
    a.mask, a.a_embedded, a.a_embedded_random, a.a_embedded_random_rec, a.content_wo, a.content_with = p(m), p(ae), p(ar), p(arr), p(cw), p(cwi)
    a.n_a = ae.numel() if ae is not None else 0
    a.n_rec = arr.numel() if arr is not None else 0
    a.n_content = cw.numel() if cw is not None else 0
    a.n_rays = R
    a.mse_on_appearance = int(bool(mse_on_appearance))
    a.coef, a.weight_kl, a.weight_rec_a, a.weight_content = float(coef), float(weight_kl), float(weight_rec_a), float(weight_content)
    a.mask_size_weight, a.mask_digit_weight = float(mask_size_weight), float(mask_digit_weight)
    a._memory_order = layouts       # inputs handed over in memory order (name -> strides): their gradients must be allocated with the same strides
    return a, keep


_loss_ws = {}


def loss_forward(args):
    lib = _lib.load()
    dev = torch.device("cuda", torch.cuda.current_device())
    if dev not in _loss_ws:
        _loss_ws[dev] = torch.empty(lib.crnerf_loss_workspace_bytes(), dtype=torch.uint8, device=dev)
    losses = torch.empty(7, dtype=torch.float32, device=dev)
    _lib.check(lib.crnerf_loss_f32(ctypes.byref(args), _lib.dev_ptr(losses), ctypes.c_void_p(_loss_ws[dev].data_ptr()), _lib.stream_ptr()),
               "crnerf_loss_f32")
    return losses


def loss_backward(args, upstream, want, strides=None):
    """want: dict name -> shape of the gradients to produce (names of struct crnerf_loss_grads without the d_ prefix); strides: name -> strides
    for the inputs loss_args handed over in memory order (their gradients are written in that order too)."""
    lib = _lib.load()
    g = _lib.LossGrads()
    out = {}
    for name, shape in want.items():
        st = (strides or {}).get(name)
        out[name] = (torch.empty_strided(tuple(shape), tuple(st), dtype=torch.float32, device=upstream.device) if st is not None
                     else torch.empty(shape, dtype=torch.float32, device=upstream.device))
        setattr(g, "d_" + name, out[name].data_ptr())
    _lib.check(lib.crnerf_loss_backward_f32(ctypes.byref(args), _lib.dev_ptr(_f32c(upstream, "upstream")), ctypes.byref(g), _lib.stream_ptr()),
               "crnerf_loss_backward_f32")
    return out


METRICS_TILE = (_lib.METRICS_TILE_H, _lib.METRICS_TILE_W)    # rows, columns of one workgroup's tile of the ROI (csrc/metrics.hip)
_metrics_ws = {}


def _chw_view(t, name):
    """(C,H,W) view of an image given as (1,C,H,W) or (C,H,W); any strides (the kernel reads the image in place)."""
    if not torch.is_tensor(t):
        raise TypeError("crnerf_amd: %s must be a tensor" % name)
    if not t.is_cuda:
        raise RuntimeError("crnerf_amd: %s is on %s; the HIP path needs GPU tensors and has no CPU fallback" % (name, t.device))
    if t.device.index != _lib._current_device():
        raise _lib._bad_tensor(t, name, torch.float32)
    if t.dtype != torch.float32:
        raise TypeError("crnerf_amd: %s must be float32, got %s" % (name, t.dtype))
    if t.dim() == 4 and t.shape[0] == 1:
        t = t[0]
    if t.dim() != 3:
        raise ValueError("crnerf_amd: %s must be (1,C,H,W) or (C,H,W), got %s" % (name, tuple(t.shape)))
    return t.detach()


def image_metrics(pred, gt, roi=None, quantize_pred=False, want_map=False):
    """crnerf_image_metrics_f32 on the region of interest roi = (x0, y0, w, h) (None: the whole image) of an image pair given as
    (1,C,H,W) or (C,H,W) views of ANY strides -- the reference's NCHW, decode_image's [H*W,3] seen as CHW, a slice of a wider image --
    read in place.  Returns (sse, ssim_sum, n, map): two 0-dim float64 device tensors (sum of squared differences, sum of the SSIM
    map), n = C*h*w, and the [C,h,w] map (None unless want_map).  quantize_pred: the prediction goes through the uint8 round trip
    of the reference's PNG files on load."""
    lib = _lib.load()
    p, g = _chw_view(pred, "image_pred"), _chw_view(gt, "image_gt")
    if p.shape != g.shape:
        raise ValueError("crnerf_amd: image_pred %s and image_gt %s differ in shape" % (tuple(p.shape), tuple(g.shape)))
    C, H, W = (int(v) for v in p.shape)
    x0, y0, w, h = (0, 0, W, H) if roi is None else (int(v) for v in roi)
    if w < 2 or h < 2 or x0 < 0 or y0 < 0 or x0 + w > W or y0 + h > H:
        raise ValueError("crnerf_amd: roi (x0=%d, y0=%d, w=%d, h=%d) must be at least 2x2 and lie inside the %dx%d image" % (x0, y0, w, h, W, H))
    a = _lib.ImageMetricsArgs()
    a.pred, a.pred_stride_c, a.pred_stride_y, a.pred_stride_x = p.data_ptr(), p.stride(0), p.stride(1), p.stride(2)
    a.gt, a.gt_stride_c, a.gt_stride_y, a.gt_stride_x = g.data_ptr(), g.stride(0), g.stride(1), g.stride(2)
    a.channels, a.width, a.height = C, W, H
    a.x0, a.y0, a.w, a.h = x0, y0, w, h
    a.quantize_pred = int(bool(quantize_pred))
    dev = p.device
    need = lib.crnerf_image_metrics_workspace_bytes(C, w, h)
    ws = _metrics_ws.get(dev)
    if ws is None or ws.numel() < need:
        ws = _metrics_ws[dev] = torch.empty(need, dtype=torch.uint8, device=dev)     # stream-ordered reuse, like the loss workspace
    out2 = torch.empty(2, dtype=torch.float64, device=dev)
    ssim_map = torch.empty((C, h, w), dtype=torch.float32, device=dev) if want_map else None
    _lib.check(lib.crnerf_image_metrics_f32(ctypes.byref(a), ctypes.c_void_p(out2.data_ptr()), _lib.dev_ptr(ssim_map, "ssim_map"),
                                            ctypes.c_void_p(ws.data_ptr()), _lib.stream_ptr()), "crnerf_image_metrics_f32")
    return out2[0], out2[1], C * h * w, ssim_map


LPIPS_CHANNELS = (64, 192, 384, 256, 256)      # channels of the five AlexNet taps (csrc/lpips.hip)
_lpips_ws = {}


def lpips_map_sizes(h, w):
    """[(h_l, w_l)] of F1..F5 for an h x w region: conv1 gives (n - 7) // 4 + 1, each 3/2 pool (m - 3) // 2 + 1 (31 -> 7 -> 3 -> 1)."""
    s1 = ((h - 7) // 4 + 1, (w - 7) // 4 + 1)
    s2 = tuple((m - 3) // 2 + 1 for m in s1)
    s3 = tuple((m - 3) // 2 + 1 for m in s2)
    return [s1, s2, s3, s3, s3]


def lpips(pred, gt, weights, roi=None, quantize_pred=False, normalize=True, want_features=False):
    """crnerf_lpips_f32 (LPIPS, AlexNet backbone; include/crnerf.h restates the definition) on the region of interest roi = (x0, y0, w, h)
    (None: the whole image; at least 31 x 31) of an image pair given as (1,3,H,W) or (3,H,W) float32 GPU views of ANY strides, read in
    place like image_metrics.  weights: a metrics.LPIPSWeights (the 17 float32 device tensors).  quantize_pred: the prediction goes
    through the uint8 round trip of the reference's PNG on load; normalize: both images are in [0,1] and go through * 2 - 1 first.
    Returns (total, per_layer, features): a 0-dim and a [5] float64 device tensor (per_layer = d_1..d_5, total their sum) and, with
    want_features, [[F1..F5 of pred], [F1..F5 of gt]] as [C,h,w] float32 tensors (None otherwise)."""
    lib = _lib.load()
    p, g = _chw_view(pred, "image_pred"), _chw_view(gt, "image_gt")
    if p.shape != g.shape:
        raise ValueError("crnerf_amd: image_pred %s and image_gt %s differ in shape" % (tuple(p.shape), tuple(g.shape)))
    C, H, W = (int(v) for v in p.shape)
    if C != 3:
        raise ValueError("crnerf_amd: lpips takes 3-channel images, got %d channels" % C)
    x0, y0, w, h = (0, 0, W, H) if roi is None else (int(v) for v in roi)
    if w < 31 or h < 31 or x0 < 0 or y0 < 0 or x0 + w > W or y0 + h > H:
        raise ValueError("crnerf_amd: roi (x0=%d, y0=%d, w=%d, h=%d) must be at least 31x31 and lie inside the %dx%d image" % (x0, y0, w, h, W, H))
    a = _lib.LpipsArgs()
    a.pred, a.pred_stride_c, a.pred_stride_y, a.pred_stride_x = p.data_ptr(), p.stride(0), p.stride(1), p.stride(2)
    a.gt, a.gt_stride_c, a.gt_stride_y, a.gt_stride_x = g.data_ptr(), g.stride(0), g.stride(1), g.stride(2)
    a.width, a.height = W, H
    a.x0, a.y0, a.w, a.h = x0, y0, w, h
    a.quantize_pred, a.normalize = int(bool(quantize_pred)), int(bool(normalize))
    for l in range(5):
        a.conv_w[l] = _lib.dev_ptr(weights.conv_w[l], "conv_w[%d]" % l)
        a.conv_b[l] = _lib.dev_ptr(weights.conv_b[l], "conv_b[%d]" % l)
        a.lin[l] = _lib.dev_ptr(weights.lin[l], "lin[%d]" % l)
    a.shift, a.scale = _lib.dev_ptr(weights.shift, "shift"), _lib.dev_ptr(weights.scale, "scale")
    dev = p.device
    need = lib.crnerf_lpips_workspace_bytes(w, h)
    ws = _lpips_ws.get(dev)
    if ws is None or ws.numel() < need:
        ws = _lpips_ws[dev] = torch.empty(need, dtype=torch.uint8, device=dev)     # stream-ordered reuse, like the metrics workspace
    out6 = torch.empty(6, dtype=torch.float64, device=dev)
    features, fptr = None, None
    if want_features:
        sizes = lpips_map_sizes(h, w)
        features = [[torch.empty((LPIPS_CHANNELS[l],) + sizes[l], dtype=torch.float32, device=dev) for l in range(5)] for _ in range(2)]
        fptr = _lib.ptr_array(features[0] + features[1], "features")
    _lib.check(lib.crnerf_lpips_f32(ctypes.byref(a), ctypes.c_void_p(out6.data_ptr()), fptr, ctypes.c_void_p(ws.data_ptr()), _lib.stream_ptr()),
               "crnerf_lpips_f32")
    return out6[5], out6[:5], features


LANCZOS_TILE = (_lib.LANCZOS_TILE_H, _lib.LANCZOS_TILE_W)   # rows, output columns of one workgroup of the horizontal pass (csrc/imageprep.hip)
LANCZOS_VBLOCK = _lib.LANCZOS_VBLOCK                         # bytes of an output row of one workgroup of the vertical pass
_lanczos_ws = {}
_lanczos_tables = {}


def _lanczos_axis(dev, in_size, out_size):
    """(k, bounds, ksize) of one axis on the device, built once per (device, size pair); (None, None, 0) for a pass that is skipped."""
    if in_size == out_size:
        return None, None, 0
    key = (dev, in_size, out_size)
    got = _lanczos_tables.get(key)
    if got is None:
        from .datasets.images import lanczos_coeffs
        k, bounds = lanczos_coeffs(in_size, out_size)
        if len(_lanczos_tables) >= 256:
            _lanczos_tables.clear()
        got = _lanczos_tables[key] = (torch.from_numpy(k).to(dev), torch.from_numpy(bounds).to(dev), int(k.shape[1]))
    return got


def lanczos_resize(img_u8, size_wh, out="u8", signed=False, dst=None):
    """crnerf_lanczos_resize_u8: PIL.Image.resize(size_wh, Image.LANCZOS) of a decoded photo, bit for bit, with the reference's tensor
    conversions fused into the store.  img_u8: contiguous uint8 [H, W, 3] on the GPU; size_wh = (w, h).
    out="u8": uint8 [h, w, 3]; "rows": float32 [h*w, 3] = ToTensor(img).view(3, -1).permute(1, 0) (the rgbs / all_rgbs layout);
    "chw": float32 [3, h, w] = ToTensor(img), with signed=True Normalize(0.5, 0.5) of it ([-1, 1], the whole_img layout).
    dst: write there instead of a fresh tensor -- contiguous, of the output's dtype and shape (a slice of rows of a larger buffer is).
    A size that equals the source's skips that pass; with both skipped the call is the conversion alone."""
    if not torch.is_tensor(img_u8) or not img_u8.is_cuda:
        raise ValueError("crnerf_amd: lanczos_resize needs a GPU tensor (got %s); the HIP path has no CPU fallback"
                         % (img_u8.device if torch.is_tensor(img_u8) else type(img_u8).__name__))
    if img_u8.dtype != torch.uint8:
        raise ValueError("crnerf_amd: lanczos_resize takes a uint8 image, got %s" % img_u8.dtype)
    if img_u8.dim() != 3 or img_u8.shape[2] != 3 or img_u8.shape[0] < 1 or img_u8.shape[1] < 1:
        raise ValueError("crnerf_amd: lanczos_resize takes an image of shape [H, W, 3], got %s" % (tuple(img_u8.shape),))
    if not img_u8.is_contiguous():
        raise ValueError("crnerf_amd: lanczos_resize takes a contiguous image")
    if img_u8.device.index != _lib._current_device():
        raise _lib._bad_tensor(img_u8, "img_u8", torch.uint8)
    if out not in ("u8", "rows", "chw") or (signed and out != "chw"):
        raise ValueError("crnerf_amd: out must be 'u8', 'rows' or 'chw' (signed=True with 'chw' only), got %r" % (out,))
    H, W = int(img_u8.shape[0]), int(img_u8.shape[1])
    w, h = (int(v) for v in size_wh)
    if w < 1 or h < 1:
        raise ValueError("crnerf_amd: lanczos_resize to a size below 1x1: %s" % ((w, h),))
    dev = img_u8.device
    shape, dtype = {"u8": ((h, w, 3), torch.uint8), "rows": ((h * w, 3), torch.float32), "chw": ((3, h, w), torch.float32)}[out]
    if dst is None:
        dst = torch.empty(shape, dtype=dtype, device=dev)
    elif (not torch.is_tensor(dst) or dst.device != dev or dst.dtype != dtype or tuple(dst.shape) != shape or not dst.is_contiguous()):
        raise ValueError("crnerf_amd: dst must be a contiguous %s tensor of shape %s on %s" % (dtype, shape, dev))
    lib = _lib.load()
    kx, bx, ksx = _lanczos_axis(dev, W, w)
    ky, by, ksy = _lanczos_axis(dev, H, h)
    need = lib.crnerf_lanczos_workspace_bytes(H, W, w, h)
    ws = _lanczos_ws.get(dev)
    if need and (ws is None or ws.numel() < need):
        ws = _lanczos_ws[dev] = torch.empty(need, dtype=torch.uint8, device=dev)     # stream-ordered reuse, like the metrics workspace
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
    _lib.check(lib.crnerf_lanczos_resize_u8(p(img_u8), H, W, w, h, p(kx), p(bx), ksx, p(ky), p(by), ksy,
                                            _lib.LANCZOS_OUT["chw_signed" if signed else out], p(dst), p(ws) if need else None, _lib.stream_ptr()),
               "crnerf_lanczos_resize_u8")
    return dst


RGBA_TILE = (_lib.RGBA_TILE_H, _lib.RGBA_TILE_W)            # rows, output columns of one workgroup of the horizontal pass (csrc/rgbaprep.hip)
RGBA_VBLOCK = _lib.RGBA_VBLOCK                               # pixels of an output row of one workgroup of the vertical pass
RGBA_MAX_RECTS = _lib.RGBA_MAX_RECTS
_rgba_ws = {}


def rgba_prepare(img_u8, size_wh, out="u8", signed=False, rects=None, colors=None, lut=None, dst=None, valid_mask=False):
    """crnerf_rgba_prepare_u8 (include/crnerf_blender.h): the Blender dataset's preparation of a decoded RGBA frame, bit for bit -- the
    occluders and the colour table of add_perturbation, PIL.Image.resize(size_wh, Image.LANCZOS) of an RGBA image (premultiplied inside, as
    Pillow does), and the white blend fused into the store.  img_u8: contiguous uint8 [H, W, 4] on the GPU; size_wh = (w, h).
    out="u8": uint8 [h, w, 4]; "rows": float32 [h*w, 3] = rgb * a + (1 - a) of ToTensor(img), pixel-major (the rgbs / all_rgbs layout);
    "chw": float32 [3, h, w] of the same blend, with signed=True Normalize(0.5, 0.5) of it ([-1, 1], the all_imgs / whole_img layout).
    rects / colors: up to RGBA_MAX_RECTS occluders, host int [n, 4] = inclusive (x0, y0, x1, y1) in source pixels and host uint8 [n, 3]; the
    last rectangle that holds a pixel wins and sets alpha 255.  lut: uint8 [3, 256] (host or device), applied to R, G, B after the occluders.
    dst: write there instead of a fresh tensor -- contiguous, of the output's dtype and shape (a slice of a larger buffer is).
    valid_mask=True: returns (out, mask) with mask bool [h*w] = alpha > 0 of the resized frame.
    A size that equals the source's skips that pass; with both skipped nothing is premultiplied: the frame's bytes pass as they are."""
    if not torch.is_tensor(img_u8) or not img_u8.is_cuda:
        raise ValueError("crnerf_amd: rgba_prepare needs a GPU tensor (got %s); the HIP path has no CPU fallback"
                         % (img_u8.device if torch.is_tensor(img_u8) else type(img_u8).__name__))
    if img_u8.dtype != torch.uint8:
        raise ValueError("crnerf_amd: rgba_prepare takes a uint8 image, got %s" % img_u8.dtype)
    if img_u8.dim() != 3 or img_u8.shape[2] != 4 or img_u8.shape[0] < 1 or img_u8.shape[1] < 1:
        raise ValueError("crnerf_amd: rgba_prepare takes an image of shape [H, W, 4], got %s" % (tuple(img_u8.shape),))
    if not img_u8.is_contiguous():
        raise ValueError("crnerf_amd: rgba_prepare takes a contiguous image")
    if img_u8.device.index != _lib._current_device():
        raise _lib._bad_tensor(img_u8, "img_u8", torch.uint8)
    if out not in ("u8", "rows", "chw") or (signed and out != "chw"):
        raise ValueError("crnerf_amd: out must be 'u8', 'rows' or 'chw' (signed=True with 'chw' only), got %r" % (out,))
    H, W = int(img_u8.shape[0]), int(img_u8.shape[1])
    w, h = (int(v) for v in size_wh)
    if w < 1 or h < 1:
        raise ValueError("crnerf_amd: rgba_prepare to a size below 1x1: %s" % ((w, h),))
    dev = img_u8.device
    n_rects, rects_np, colors_np = 0, None, None
    if rects is not None and len(rects) > 0:
        rects_np = np.ascontiguousarray(np.asarray(rects, dtype=np.int32).reshape(-1, 4))
        if colors is None:
            raise ValueError("crnerf_amd: rgba_prepare: rects come with colors")
        colors_np = np.ascontiguousarray(np.asarray(colors, dtype=np.uint8).reshape(-1, 3))
        n_rects = int(rects_np.shape[0])
        if colors_np.shape[0] != n_rects or n_rects > RGBA_MAX_RECTS:
            raise ValueError("crnerf_amd: rgba_prepare takes up to %d rectangles with one colour each, got %d and %d"
                             % (RGBA_MAX_RECTS, n_rects, colors_np.shape[0]))
    if lut is not None:
        lut = torch.as_tensor(lut)
        if lut.dtype != torch.uint8 or tuple(lut.shape) != (3, 256):
            raise ValueError("crnerf_amd: lut must be uint8 [3, 256], got %s %s" % (lut.dtype, tuple(lut.shape)))
        lut = lut.to(dev).contiguous()
    shape, dtype = {"u8": ((h, w, 4), torch.uint8), "rows": ((h * w, 3), torch.float32), "chw": ((3, h, w), torch.float32)}[out]
    if dst is None:
        dst = torch.empty(shape, dtype=dtype, device=dev)
    elif (not torch.is_tensor(dst) or dst.device != dev or dst.dtype != dtype or tuple(dst.shape) != shape or not dst.is_contiguous()):
        raise ValueError("crnerf_amd: dst must be a contiguous %s tensor of shape %s on %s" % (dtype, shape, dev))
    mask = torch.empty(h * w, dtype=torch.bool, device=dev) if valid_mask else None
    lib = _lib.load()
    kx, bx, ksx = _lanczos_axis(dev, W, w)
    ky, by, ksy = _lanczos_axis(dev, H, h)
    need = lib.crnerf_rgba_prepare_workspace_bytes(H, W, w, h)
    ws = _rgba_ws.get(dev)
    if need and (ws is None or ws.numel() < need):
        ws = _rgba_ws[dev] = torch.empty(need, dtype=torch.uint8, device=dev)     # stream-ordered reuse, like the metrics workspace
    p = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
    a = _lib.RgbaPrepareArgs()
    a.src, a.H, a.W, a.w, a.h = p(img_u8), H, W, w, h
    a.kx, a.bounds_x, a.ky, a.bounds_y, a.ksize_x, a.ksize_y = p(kx), p(bx), p(ky), p(by), ksx, ksy
    a.n_rects, a.out_mode = n_rects, _lib.RGBA_OUT["chw_signed" if signed else out]
    a.rects = rects_np.ctypes.data if n_rects else None
    a.colors = colors_np.ctypes.data if n_rects else None
    a.lut, a.dst, a.valid_mask, a.workspace = p(lut), p(dst), p(mask), p(ws) if need else None
    _lib.check(lib.crnerf_rgba_prepare_u8(ctypes.byref(a), _lib.stream_ptr()), "crnerf_rgba_prepare_u8")
    return (dst, mask) if valid_mask else dst


_scene_ws = {}


def scene_bounds(xyz, w2c_row2, q_lo=0.1, q_hi=99.9):
    """crnerf_scene_bounds_f64: per image, np.percentile(depth[depth > 0], q_lo) and (..., q_hi) of the camera-space depth
    ((x r20 + y r21) + z r22) + t2 of every point (include/crnerf.h states the arithmetic; read_meta :133-137 in the reference).
    xyz: float64 [P, 3], w2c_row2: float64 [N, 4] = (r20, r21, r22, t2) per image, both contiguous on the GPU.  Returns (nears float64 [N],
    fars float64 [N], counts int32 [N]); an image with nothing in front of it has count 0 and NaN bounds."""
    for t, name, cols in ((xyz, "xyz", 3), (w2c_row2, "w2c_row2", 4)):
        if not torch.is_tensor(t) or not t.is_cuda:
            raise ValueError("crnerf_amd: scene_bounds needs GPU tensors (%s is %s); the HIP path has no CPU fallback"
                             % (name, t.device if torch.is_tensor(t) else type(t).__name__))
        if t.dtype != torch.float64:
            raise TypeError("crnerf_amd: scene_bounds takes float64 (%s is %s): the reference holds the sparse model and the poses in float64"
                            % (name, t.dtype))
        if t.dim() != 2 or t.shape[1] != cols:
            raise ValueError("crnerf_amd: %s must have shape [*, %d], got %s" % (name, cols, tuple(t.shape)))
    n_points, n_images = int(xyz.shape[0]), int(w2c_row2.shape[0])
    if n_images < 1:
        raise ValueError("crnerf_amd: scene_bounds needs at least one image")
    if n_points >= 2 ** 31:
        raise ValueError("crnerf_amd: scene_bounds takes fewer than 2^31 points, got %d" % n_points)
    q_lo, q_hi = float(q_lo), float(q_hi)
    if not (0.0 <= q_lo <= q_hi <= 100.0):
        raise ValueError("crnerf_amd: scene_bounds needs 0 <= q_lo <= q_hi <= 100, got (%r, %r)" % (q_lo, q_hi))
    lib = _lib.load()
    dev = xyz.device
    nears = torch.empty(n_images, dtype=torch.float64, device=dev)
    fars = torch.empty(n_images, dtype=torch.float64, device=dev)
    counts = torch.empty(n_images, dtype=torch.int32, device=dev)
    need = lib.crnerf_scene_bounds_workspace_bytes(n_images, n_points)
    ws = _scene_ws.get(dev)
    if need and (ws is None or ws.numel() < need):
        ws = _scene_ws[dev] = torch.empty(need, dtype=torch.uint8, device=dev)     # stream-ordered reuse, like the metrics workspace
    _lib.check(lib.crnerf_scene_bounds_f64(_lib.dev_ptr(xyz, "xyz", torch.float64) if n_points else None, n_points,
                                           _lib.dev_ptr(w2c_row2, "w2c_row2", torch.float64), n_images, q_lo, q_hi,
                                           _lib.dev_ptr(nears, "nears", torch.float64), _lib.dev_ptr(fars, "fars", torch.float64),
                                           _lib.dev_ptr(counts, "counts", torch.int32), ctypes.c_void_p(ws.data_ptr()) if need else None,
                                           _lib.stream_ptr()), "crnerf_scene_bounds_f64")
    return nears, fars, counts


def grid_sample_batch(all_rays, all_rgbs, row_offset, img_w, img_h, side, w_lin, h_lin, scale, h_offset, w_offset, rounding="floor"):
    """rounding: how a lattice node becomes a pixel -- "floor" (the Phototourism batcher) or "round" (the Blender batcher's .round(), half to even)."""
    if rounding not in ("floor", "round"):
        raise ValueError("crnerf_amd: rounding must be 'floor' or 'round', got %r" % (rounding,))
    lib = _lib.load()
    all_rays, all_rgbs = _f32c(all_rays, "all_rays"), _f32c(all_rgbs, "all_rgbs")
    if all_rays.dim() != 2 or all_rays.shape[1] < 9 or all_rgbs.dim() != 2 or all_rgbs.shape[1] != 3:
        raise ValueError("crnerf_amd: all_rays must be [N,>=9] and all_rgbs [N,3]")
    w_lin, h_lin = _f32c(w_lin, "w_lin"), _f32c(h_lin, "h_lin")
    dev, n = all_rays.device, side * side
    out = {"rays": torch.empty(n, 8, device=dev), "ts": torch.empty(n, dtype=torch.int64, device=dev), "rgbs": torch.empty(n, 3, device=dev),
           "rgb_idx": torch.empty(n, dtype=torch.int64, device=dev), "uv_sample": torch.empty(n, 2, device=dev)}
    a = _lib.BatchArgs()
    a.all_rays, a.ray_stride, a.all_rgbs, a.row_offset = all_rays.data_ptr(), all_rays.stride(0), all_rgbs.data_ptr(), int(row_offset)
    a.img_w, a.img_h, a.side = int(img_w), int(img_h), int(side)
    a.w_lin, a.h_lin = w_lin.data_ptr(), h_lin.data_ptr()
    a.scale, a.h_offset, a.w_offset = float(scale), float(h_offset), float(w_offset)
    a.rays, a.ts, a.rgbs, a.rgb_idx, a.uv_sample = (out[k].data_ptr() for k in ("rays", "ts", "rgbs", "rgb_idx", "uv_sample"))
    if rounding == "round":
        _lib.check(lib.crnerf_grid_sample_batch_round_f32(ctypes.byref(a), _lib.stream_ptr()), "crnerf_grid_sample_batch_round_f32")
    else:
        _lib.check(lib.crnerf_grid_sample_batch_f32(ctypes.byref(a), _lib.stream_ptr()), "crnerf_grid_sample_batch_f32")
    return out


# ---------------------------------------------------------------- transient-mask network operators (csrc/cgnet.hip)
def _chw(t, name):
    """[1,C,H,W] or [C,H,W] fp32 device tensor -> contiguous, with its (C, H, W)."""
    t = _f32c(t, name)
    if t.dim() == 4:
        if t.shape[0] != 1:
            raise ValueError("crnerf_amd: %s: the mask network runs on one image (batch 1), got batch %d" % (name, t.shape[0]))
    elif t.dim() != 3:
        raise ValueError("crnerf_amd: %s must be [1,C,H,W] or [C,H,W]" % name)
    return t, tuple(t.shape[-3:])


def _geom(x_shape, w, stride, padding, dilation, groups):
    C, H, W = x_shape
    cout, cpg, k, k2 = w.shape
    if k != k2:
        raise ValueError("crnerf_amd: conv2d: square kernels only")
    if groups == 1:
        if cpg != C:
            raise ValueError("crnerf_amd: conv2d: weight expects %d input channels, got %d" % (cpg, C))
    elif not (groups == C == cout and cpg == 1):
        raise ValueError("crnerf_amd: conv2d: groups must be 1 or depth-wise (groups = cin = cout)")
    g = _lib.ConvGeom(C, cout, H, W, k, stride, padding, dilation, int(groups != 1))
    Ho = (H + 2 * padding - dilation * (k - 1) - 1) // stride + 1
    Wo = (W + 2 * padding - dilation * (k - 1) - 1) // stride + 1
    return g, Ho, Wo


def conv2d(x, w, stride=1, padding=0, dilation=1, groups=1):
    """F.conv2d(x, w, None, stride, padding, dilation, groups) for batch 1 (groups = 1 or depth-wise)."""
    lib = _lib.load()
    x, shp = _chw(x, "x")
    w = _f32c(w, "weight")
    g, Ho, Wo = _geom(shp, w, stride, padding, dilation, groups)
    y = torch.empty(1, w.shape[0], Ho, Wo, device=x.device)
    _lib.check(lib.crnerf_conv2d_f32(ctypes.byref(g), _lib.dev_ptr(x), _lib.dev_ptr(w), _lib.dev_ptr(y), _lib.stream_ptr()), "crnerf_conv2d_f32")
    return y


def conv2d_backward(x, w, d_y, stride=1, padding=0, dilation=1, groups=1, want_dx=True):
    lib = _lib.load()
    x, shp = _chw(x, "x")
    w, d_y = _f32c(w, "weight"), _f32c(d_y, "d_y")
    g, _, _ = _geom(shp, w, stride, padding, dilation, groups)
    dx = torch.empty_like(x) if want_dx else None
    dw = torch.empty_like(w)
    _lib.check(lib.crnerf_conv2d_backward_f32(ctypes.byref(g), _lib.dev_ptr(x), _lib.dev_ptr(w), _lib.dev_ptr(d_y), _lib.dev_ptr(dx), _lib.dev_ptr(dw),
                                              _lib.stream_ptr()), "crnerf_conv2d_backward_f32")
    return dx, dw


def bn_prelu(x, gamma, beta, alpha, eps, training, running_mean=None, running_var=None, update=None):
    """BatchNorm2d + PReLU.  Returns (y, mean, invstd, var_unbiased); eval mode reads the running statistics.
    update=(momentum, num_batches_tracked or None) in training mode: the momentum update of running_mean / running_var (and the step
    counter) happens in the SAME launch (crnerf_bn_prelu_train_f32) instead of five element-wise launches per layer."""
    lib = _lib.load()
    x, (C, H, W) = _chw(x, "x")
    y = torch.empty_like(x)
    if training and update is not None:
        mean, invstd, var_u = (torch.empty(C, device=x.device) for _ in range(3))
        momentum, nbt = update
        for t, n in ((running_mean, "running_mean"), (running_var, "running_var")):
            if t.dtype != torch.float32 or not t.is_contiguous() or not t.is_cuda:
                raise ValueError("crnerf_amd: %s must be a contiguous float32 GPU buffer" % n)
        _lib.check(lib.crnerf_bn_prelu_train_f32(_lib.dev_ptr(x), _lib.dev_ptr(_f32c(gamma, "bn.weight")), _lib.dev_ptr(_f32c(beta, "bn.bias")),
                                                 _lib.dev_ptr(_f32c(alpha, "act.weight")), _lib.dev_ptr(mean), _lib.dev_ptr(invstd), _lib.dev_ptr(var_u),
                                                 _lib.dev_ptr(y), _lib.dev_ptr(running_mean), _lib.dev_ptr(running_var),
                                                 ctypes.c_void_p(nbt.data_ptr()) if nbt is not None else None, float(momentum), C, H * W, float(eps),
                                                 _lib.stream_ptr()), "crnerf_bn_prelu_train_f32")
        return y, mean, invstd, var_u
    if training:
        mean, invstd, var_u = (torch.empty(C, device=x.device) for _ in range(3))
    else:
        mean, invstd, var_u = _f32c(running_mean, "running_mean"), torch.rsqrt(_f32c(running_var, "running_var") + eps), None
    _lib.check(lib.crnerf_bn_prelu_f32(_lib.dev_ptr(x), _lib.dev_ptr(_f32c(gamma, "bn.weight")), _lib.dev_ptr(_f32c(beta, "bn.bias")),
                                       _lib.dev_ptr(_f32c(alpha, "act.weight")), _lib.dev_ptr(mean), _lib.dev_ptr(invstd), _lib.dev_ptr(var_u),
                                       _lib.dev_ptr(y), C, H * W, float(eps), int(bool(training)), _lib.stream_ptr()), "crnerf_bn_prelu_f32")
    return y, mean, invstd, var_u


def bn_prelu_backward(x, gamma, beta, alpha, mean, invstd, d_y, training):
    lib = _lib.load()
    x, (C, H, W) = _chw(x, "x")
    d_y = _f32c(d_y, "d_y")
    dx = torch.empty_like(x)
    dg, db, da = (torch.empty(C, device=x.device) for _ in range(3))
    _lib.check(lib.crnerf_bn_prelu_backward_f32(_lib.dev_ptr(x), _lib.dev_ptr(_f32c(gamma, "bn.weight")), _lib.dev_ptr(_f32c(beta, "bn.bias")),
                                                _lib.dev_ptr(_f32c(alpha, "act.weight")), _lib.dev_ptr(mean), _lib.dev_ptr(invstd), _lib.dev_ptr(d_y),
                                                _lib.dev_ptr(dx), _lib.dev_ptr(dg), _lib.dev_ptr(db), _lib.dev_ptr(da), C, H * W, int(bool(training)),
                                                _lib.stream_ptr()), "crnerf_bn_prelu_backward_f32")
    return dx, dg, db, da


def avgpool3s2(x):
    """nn.AvgPool2d(3, stride=2, padding=1)."""
    lib = _lib.load()
    x, (C, H, W) = _chw(x, "x")
    y = torch.empty(1, C, (H - 1) // 2 + 1, (W - 1) // 2 + 1, device=x.device)
    _lib.check(lib.crnerf_avgpool3s2_f32(_lib.dev_ptr(x), _lib.dev_ptr(y), C, H, W, 0, _lib.stream_ptr()), "crnerf_avgpool3s2_f32")
    return y


def avgpool3s2_backward(d_y, in_shape):
    lib = _lib.load()
    d_y = _f32c(d_y, "d_y")
    C, H, W = in_shape
    dx = torch.empty(1, C, H, W, device=d_y.device)
    _lib.check(lib.crnerf_avgpool3s2_f32(_lib.dev_ptr(d_y), _lib.dev_ptr(dx), C, H, W, 1, _lib.stream_ptr()), "crnerf_avgpool3s2_f32")
    return dx


def fglo(x, w1, b1, w2, b2):
    """FGlo: x * sigmoid(fc2(relu(fc1(mean_hw(x))))).  Returns (y, stats) -- stats is what the backward needs."""
    lib = _lib.load()
    x, (C, H, W) = _chw(x, "x")
    R = w1.shape[0]
    y, stats = torch.empty_like(x), torch.empty(2 * C + R, device=x.device)
    _lib.check(lib.crnerf_fglo_f32(_lib.dev_ptr(x), _lib.dev_ptr(_f32c(w1, "fc.0.weight")), _lib.dev_ptr(_f32c(b1, "fc.0.bias")),
                                   _lib.dev_ptr(_f32c(w2, "fc.2.weight")), _lib.dev_ptr(_f32c(b2, "fc.2.bias")), _lib.dev_ptr(stats), _lib.dev_ptr(y),
                                   C, R, H * W, _lib.stream_ptr()), "crnerf_fglo_f32")
    return y, stats


def fglo_backward(x, w1, w2, stats, d_y):
    lib = _lib.load()
    x, (C, H, W) = _chw(x, "x")
    d_y = _f32c(d_y, "d_y")
    R = w1.shape[0]
    dev = x.device
    dx, dw1, db1, dw2, db2 = torch.empty_like(x), torch.empty(R, C, device=dev), torch.empty(R, device=dev), torch.empty(C, R, device=dev), \
        torch.empty(C, device=dev)
    scratch = torch.empty(2 * C, device=dev)
    _lib.check(lib.crnerf_fglo_backward_f32(_lib.dev_ptr(x), _lib.dev_ptr(_f32c(w1, "fc.0.weight")), _lib.dev_ptr(_f32c(w2, "fc.2.weight")),
                                            _lib.dev_ptr(stats), _lib.dev_ptr(d_y), _lib.dev_ptr(scratch), _lib.dev_ptr(dx), _lib.dev_ptr(dw1),
                                            _lib.dev_ptr(db1), _lib.dev_ptr(dw2), _lib.dev_ptr(db2), C, R, H * W, _lib.stream_ptr()),
               "crnerf_fglo_backward_f32")
    return dx, dw1, db1, dw2, db2


def bilinear_gather(x, size, idx=None, sigmoid=False):
    """F.interpolate(x[1,1,h,w], size, mode='bilinear', align_corners=False) (then sigmoid), at pixels idx (None: all, as [1,1,Ho,Wo])."""
    lib = _lib.load()
    x, (C, h, w) = _chw(x, "x")
    if C != 1:
        raise ValueError("crnerf_amd: bilinear_gather: one channel expected (the mask), got %d" % C)
    Ho, Wo = int(size[0]), int(size[1])
    if idx is None:
        out, n = torch.empty(1, 1, Ho, Wo, device=x.device), Ho * Wo
    else:
        idx = idx.contiguous()
        out, n = torch.empty(idx.numel(), device=x.device), idx.numel()
    _lib.check(lib.crnerf_bilinear_gather_f32(_lib.dev_ptr(x), h, w, Ho, Wo, _lib.dev_ptr(idx, "idx", torch.int64), n, int(bool(sigmoid)),
                                              _lib.dev_ptr(out), _lib.stream_ptr()), "crnerf_bilinear_gather_f32")
    return out


def bilinear_gather_backward(out, d_out, in_hw, size, idx=None, sigmoid=False):
    lib = _lib.load()
    h, w = in_hw
    Ho, Wo = int(size[0]), int(size[1])
    d_out = _f32c(d_out, "d_out")
    n = d_out.numel()
    d_in = torch.empty(1, 1, h, w, device=d_out.device)
    _lib.check(lib.crnerf_bilinear_gather_backward_f32(_lib.dev_ptr(out) if sigmoid else None, _lib.dev_ptr(d_out), h, w, Ho, Wo,
                                                       _lib.dev_ptr(idx.contiguous(), "idx", torch.int64) if idx is not None else None, n,
                                                       int(bool(sigmoid)), _lib.dev_ptr(d_in), _lib.stream_ptr()), "crnerf_bilinear_gather_backward_f32")
    return d_in


# ---------------------------------------------------------------- the mask network of a training step as two calls (csrc/cgnet_chain.hip)
def cgnet_forward_train(image, params, running_mean, running_var, num_batches_tracked, momentum, eps):
    """Context_Guided_Network(classes=1, M=2, N=2).forward in train mode (lightweight_seg.py:274-368): image[1,C,H,W] -> (mask[1,1,H,W], saved).
    params: the 76 tensors in state_dict order; running_mean / running_var / num_batches_tracked: the 14 BatchNorm layers' buffers (updated)."""
    lib = _lib.load()
    image, (C, H, W) = _chw(image, "image")
    if len(params) != lib.crnerf_cgnet_param_count() or len(running_mean) != lib.crnerf_cgnet_bn_count():
        raise ValueError("crnerf_amd: cgnet_forward_train takes %d parameters and %d BatchNorm layers" % (lib.crnerf_cgnet_param_count(), lib.crnerf_cgnet_bn_count()))
    saved = torch.empty(lib.crnerf_cgnet_arena_bytes(C, H, W) // 4, device=image.device)
    mask = torch.empty(1, 1, H, W, device=image.device)
    nbt = (ctypes.c_void_p * len(running_mean))()
    for i, t in enumerate(num_batches_tracked):
        if t is not None:
            if not t.is_cuda or t.dtype != torch.int64:
                raise ValueError("crnerf_amd: num_batches_tracked must be an int64 GPU buffer")
            nbt[i] = t.data_ptr()
    _lib.check(lib.crnerf_cgnet_forward_train_f32(_lib.dev_ptr(image), C, H, W, _lib.ptr_array(params, "params"), _lib.ptr_array(running_mean, "running_mean"),
                                                  _lib.ptr_array(running_var, "running_var"), nbt, float(momentum), float(eps), _lib.dev_ptr(saved),
                                                  _lib.dev_ptr(mask), _lib.stream_ptr()), "crnerf_cgnet_forward_train_f32")
    return mask, saved


def cgnet_backward(image, params, saved, mask, d_mask):
    """-> the 76 parameter gradients (views of one buffer, shapes of `params`)."""
    lib = _lib.load()
    image, (C, H, W) = _chw(image, "image")
    d_mask = _f32c(d_mask, "d_mask")
    scratch = torch.empty_like(saved)
    sizes = [p.numel() for p in params]
    grads = [g.view(p.shape) for g, p in zip(torch.empty(sum(sizes), device=image.device).split(sizes), params)]
    _lib.check(lib.crnerf_cgnet_backward_f32(_lib.dev_ptr(image), C, H, W, _lib.ptr_array(params, "params"), _lib.dev_ptr(saved), _lib.dev_ptr(mask),
                                             _lib.dev_ptr(d_mask), _lib.dev_ptr(scratch), _lib.ptr_array(grads, "grads"), _lib.stream_ptr()),
               "crnerf_cgnet_backward_f32")
    return grads

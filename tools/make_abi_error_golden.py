"""Records tests/golden/abi_errors.json: the return code and the crnerf_last_error() text of every argument check of csrc/abi.hip and of the
launch layer behind it (csrc/launch.h and the render / MLP launchers: sample counts, saved-row offset limits, the repair grids).  Run it on a
machine WITHOUT a GPU, with the library whose messages are the contract (the abi.hip cases in the tree were recorded from the build before the
boundary helpers -- fail / all_set / pack_entry / forward_entry / to_render_args ... -- replaced the hand-copied checks, the launch-layer cases
from the build before launch.h replaced the launchers' own copies):

    CRNERF_LIB_PATH=path/to/libcrnerf_parent.so python tools/make_abi_error_golden.py [--out FILE]

Every entry point has a BASE call that is never issued itself: dummy non-null pointers, sizes of 1, flags of 0 -- a call that would pass validation.
A case is the base with one mutation that validation refuses (or the empty-input no-op: n == 0 with every pointer NULL returns 0).  The dummy
pointers are addresses inside one page-sized host buffer; every `T* const*` argument is a real host array of 512 pointers (the library reads those
on the host); struct arguments are real ctypes structures.  A case that comes back as CRNERF_ERR_HIP, or as 0 without being marked a no-op, got
through validation to a launch: the tool refuses to record it, and tests/test_abi_errors_host.py refuses a fixture that holds one, because on a
GPU machine that call would launch on the dummy pointers.  The test module imports its cases from here, so both always issue the same calls.

Before every case the error text is set by one fixed refused call (PRIME), so a no-op's recorded text is that one: a success leaves it alone.

Checks that no case reaches:
  * check_launch, ensure_dynamic_lds, zero_acts_range, crnerf_stream_destroy's failure and hipExtStreamCreateWithCUMask's: they need the HIP runtime
    to fail;
  * of the launchers: "no fine model" (abi.hip refuses a missing packed_fine first), the training twins' NULL saved state (abi.hip's own REQUIREs
    come first), the lean and fine-only refusals of render_fused16.hip / render_fused_bf16p.hip (abi.hip checks the same conditions under its own
    texts) and the fp16 build's "inference kernel only" (no entry point routes there); the 3.9 M point limit of the two data-gradient launchers
    is not recorded either (launch_mlp_backward may touch the scratch buffer before it gets there);
  * behind the seven render entries of crnerf_lean.h / crnerf_lean_composite.h: all of launch.h's check_sample_counts and the launchers' own
    "N_importance must be 0" / "must be in [1, 256]" -- abi.hip's ranges for these entries ([3, 256] and [1, 256]; [2, 256] and 0 for the
    coarse-weights ones) come first and are no wider; what is reachable is the repair launch's one-workgroup-per-quad limit;
  * the saved-row limit of crnerf_render_rays_train_f32: that launcher has none, the call would go on to a launch;
  * crnerf_stream_create_cu_share's range check and crnerf_cus_per_xcd: they query the device before validating (only the NULL `stream` case is here);
  * crnerf_scene_bounds_f64 "workspace is NULL": scene_bounds_workspace_bytes() is 0 for every size;
  * the phase-dependent pointers of the three backward entries are covered from the refusing side only (a phase that does not read a pointer
    still refuses the next missing one): the accepting side is a launch.
crnerf_peer_* lives outside abi.hip."""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GOLDEN = os.path.join(ROOT, "tests", "golden", "abi_errors.json")
ERR_HIP = -10
PRIME = ("crnerf_pack_h2_status", "packed_h2 is NULL")      # the refused call in front of every case, and the text it leaves

_PAGE = ctypes.create_string_buffer(2 * 4096)
PTR = (ctypes.addressof(_PAGE) + 4095) // 4096 * 4096 + 256          # the dummy pointer: inside the page, 16-byte aligned
LIST_LEN = 512


class _P:       # a dummy non-null pointer
    pass


class _L:       # a host array of LIST_LEN dummy pointers
    pass


class S:
    """A struct argument: the ctypes class and its base fields (P: the dummy pointer; a c_void_p array field takes P for every element)."""

    def __init__(self, name, **fields):
        self.name, self.fields = name, fields


P, L = _P(), _L()
NAN, INF = float("nan"), float("inf")

RENDER_OUT = dict(weights_coarse=P, feature_coarse=P, depth_coarse=P, weights_fine=P, feature_fine=P, depth_fine=P)
RENDER = S("RenderArgs", packed_coarse=P, packed_fine=P, rays=P, n_rays=1, n_samples=1, n_importance=1, **RENDER_OUT)
RENDER_TRAIN = S("RenderArgs", z_fine=P, **RENDER.fields)
RENDER_FINE = S("RenderArgs", packed_fine=P, rays=P, n_rays=1, n_samples=1, n_importance=1, weights_coarse=P, weights_fine=P, feature_fine=P, depth_fine=P)
RENDER_LEAN = S("RenderArgs", packed_coarse=P, packed_fine=P, rays=P, n_rays=1, n_samples=3, n_importance=1, feature_fine=P, depth_fine=P)
LOSS = S("LossArgs", rgb_coarse=P, targets=P, n_rays=1)
BATCH = S("BatchArgs", all_rays=P, all_rgbs=P, w_lin=P, h_lin=P, rays=P, ts=P, rgbs=P, rgb_idx=P, uv_sample=P, ray_stride=9, img_w=1, img_h=1, side=1)
METRICS = S("ImageMetricsArgs", pred=P, gt=P, channels=1, width=2, height=2, x0=0, y0=0, w=2, h=2)
LPIPS = S("LpipsArgs", pred=P, gt=P, width=31, height=31, x0=0, y0=0, w=31, h=31, conv_w=P, conv_b=P, lin=P, shift=P, scale=P)
GEOM = S("ConvGeom", cin=1, cout=1, H=1, W=1, k=1, stride=1, pad=0, dil=1, depthwise=0)

MLP, ENC, DEC, CG, BN = 24, 14, 22, 76, 14      # CRNERF_MLP_TENSORS, _ENCODER_TENSORS, _DECODER_TENSORS, crnerf_cgnet_param_count(), _bn_count()
BF16, BF16X3, F16X2, DGRAD, WGRAD = 1, 2, 4, 8, 16     # CRNERF_BWD_*

CASES = []      # (entry, label, base, mutation, is_noop)
BASES = {}


def entry(name, **base):
    BASES[name] = base
    return name


def case(e, label, **mut):
    CASES.append((e, label, mut, False))


def noop(e, label, **mut):
    """The empty-input no-op: `mut` on top of every pointer argument (and every pointer field of a struct argument) NULL."""
    CASES.append((e, label, mut, True))


def nulls(e, *names):
    for n in names:
        CASES.append((e, "%s=NULL" % n, {n: None}, False))


def holes(e, name, n, *more):
    """First and last entry of an n-pointer list NULL."""
    for i in (0, n - 1) + more:
        CASES.append((e, "%s[%d]=NULL" % (name, i), {"%s[%d]" % (name, i): None}, False))


def bad(e, name, *values):
    for v in values:
        CASES.append((e, "%s=%r" % (name, v), {name: v}, False))


# ---- streams, packs
e = entry("crnerf_stream_create_cu_share", stream=L, first=0, count=1)
nulls(e, "stream")
noop(entry("crnerf_stream_destroy", stream=P), "NULL stream")
nulls(entry("crnerf_pack_h2_status", packed_h2=P, stream=None), "packed_h2")
for e in ("crnerf_pack_mlp_weights", "crnerf_pack_mlp_weights_t", "crnerf_pack_mlp_weights_mixed", "crnerf_pack_mlp_weights_t_x3", "crnerf_pack_mlp_weights_t_h2",
          "crnerf_pack_mlp_weights_x3", "crnerf_pack_mlp_weights_h2", "crnerf_pack_mlp_weights_h2_async", "crnerf_pack_mlp_weights_bf16", "crnerf_pack_mlp_weights_f16"):
    entry(e, tensors=L, packed=P, stream=None)
    nulls(e, "tensors", "packed")
    holes(e, "tensors", MLP, 11)

# ---- the MLP alone
e = entry("crnerf_mlp_forward_train_f32", packed=P, x=P, out=P, acts=P, n=1, stream=None)
nulls(e, "packed", "x", "out", "acts")
noop(e, "n=0", n=0)
for e in ("crnerf_mlp_forward_f32", "crnerf_mlp_forward_f32x3", "crnerf_mlp_forward_f32h2", "crnerf_mlp_forward_f32x3_repair", "crnerf_mlp_forward_bf16",
          "crnerf_mlp_forward_f16"):
    entry(e, packed=P, x=P, out=P, n=1, sigma_only=0, stream=None)
    nulls(e, "packed", "x", "out")
    bad(e, "n", -1)
    noop(e, "n=0", n=0)

e = entry("crnerf_mlp_backward_f32", packed_t=P, x=P, out=P, d_out=P, acts=P, scratch=P, grads=L, n=1, stream=None)
nulls(e, "acts", "scratch", "packed_t", "out", "d_out", "x", "grads")
holes(e, "grads", MLP)
noop(e, "n=0", n=0)
for e, pk, modes in (("crnerf_mlp_backward_ex_f32", dict(packed_t=P), BF16 | BF16X3), ("crnerf_mlp_backward_x3_f32", dict(packed_t=P), BF16 | BF16X3),
                     ("crnerf_mlp_backward_h2_f32", dict(packed_t=P, packed_t_x3=P), BF16 | BF16X3 | F16X2)):
    entry(e, **pk, x=P, out=P, d_out=P, acts=P, scratch=P, grads=L, n=1, flags=0, stream=None)
    nulls(e, "acts", "scratch", "packed_t", "out", "d_out", "x", "grads")
    holes(e, "grads", MLP)
    bad(e, "flags", 32, 64 | BF16, BF16 | BF16X3)
    if modes & F16X2:
        bad(e, "flags", BF16 | F16X2, BF16X3 | F16X2 | DGRAD)
    else:
        bad(e, "flags", F16X2)                              # a mode of the h2 entry only: an unknown bit here
    # a phase that does not read a pointer skips it and refuses the next missing one
    case(e, "dgrad: x and grads are not read", flags=DGRAD, x=None, grads=None, packed_t=None)
    case(e, "dgrad: out", flags=DGRAD, x=None, grads=None, out=None)
    case(e, "dgrad: d_out", flags=DGRAD | BF16, x=None, grads=None, d_out=None)
    case(e, "wgrad: the pack, out and d_out are not read", flags=WGRAD, packed_t=None, out=None, d_out=None, x=None)
    case(e, "wgrad: grads", flags=WGRAD | BF16X3, packed_t=None, out=None, d_out=None, grads=None)
    case(e, "wgrad: a gradient", flags=WGRAD, packed_t=None, out=None, d_out=None, **{"grads[5]": None})
    case(e, "both phase bits: both run", flags=DGRAD | WGRAD, x=None)
    case(e, "both phase bits: both run, the pack", flags=DGRAD | WGRAD, packed_t=None)
    case(e, "acts before the phases", flags=WGRAD, acts=None, x=None)
    noop(e, "n=0", n=0)

e = entry("crnerf_mlp_forward_train_mixed_f32", tensors=L, packed=P, x=P, out=P, acts=P, n=1, stream=None)
nulls(e, "tensors", "packed", "x", "out", "acts")
bad(e, "n", -1)
holes(e, "tensors", MLP)
noop(e, "n=0", n=0)
e = entry("crnerf_mlp_backward_mixed_f32", tensors=L, packed=P, x=P, out=P, d_out=P, acts=P, scratch=P, grads=L, n=1, stream=None)
nulls(e, "tensors", "packed", "x", "out", "d_out", "acts", "scratch", "grads")
holes(e, "tensors", MLP)
holes(e, "grads", MLP)
noop(e, "n=0", n=0)
e = entry("crnerf_mlp_backward_mixed_ex_f32", tensors=L, packed=P, out=P, d_out=P, acts=P, scratch=P, grads=L, n=1, acts_layout=0, stream=None)
nulls(e, "tensors", "packed", "out", "d_out", "acts", "scratch", "grads")
bad(e, "acts_layout", -1, 2)
holes(e, "tensors", MLP)
holes(e, "grads", MLP)
noop(e, "n=0", n=0)

# ---- the stand-alone stages
e = entry("crnerf_posenc_f32", x=P, out=P, n=1, n_freqs=1, stream=None)
nulls(e, "x", "out")
bad(e, "n", -1)
noop(e, "n=0", n=0)
e = entry("crnerf_embed_points_f32", rays=P, z=P, dir_emb=P, x=P, n_rays=1, n_samples=1, stream=None)
nulls(e, "rays", "z", "dir_emb", "x")
bad(e, "n_rays", -1)
bad(e, "n_samples", -1)
noop(e, "n_rays=0", n_rays=0)
noop(e, "n_samples=0", n_samples=0)
e = entry("crnerf_composite_f32", raw=P, z=P, noise=None, noise_std=0.0, weights=P, feature=P, depth=P, R=1, N=1, stream=None)
nulls(e, "raw", "z", "weights", "feature", "depth")
bad(e, "R", -1)
noop(e, "R=0", R=0)
e = entry("crnerf_composite_backward_f32", raw=P, z=P, noise=None, noise_std=0.0, d_feature=P, d_depth=None, d_weights=None, d_raw=P, R=1, N=1, stream=None)
nulls(e, "raw", "z", "d_feature", "d_raw")
bad(e, "R", -1)
noop(e, "R=0", R=0)
e = entry("crnerf_sample_pdf_merge_f32", z_coarse=P, weights_coarse=P, u=None, u_stride=0, z_sorted=P, z_samples=None, R=1, Nc=1, Ni=1, stream=None)
nulls(e, "z_coarse", "weights_coarse", "z_sorted")
bad(e, "R", -1)
noop(e, "R=0", R=0)
e = entry("crnerf_rng_fill_f32", out=P, n_rays=1, n=1, seed=0, stream_id=0, ray_offset=0, stream=None)
nulls(e, "out")
bad(e, "n_rays", -1)
bad(e, "n", -1)
bad(e, "stream_id", -1, 4)
noop(e, "n_rays=0", n_rays=0)
noop(e, "n=0", n=0)


# ---- the fused renderers
def render_checks(e, pair):
    """What render_entry refuses under the RENDER_RAYS descriptor (the inference entries and, behind their own checks, the training twins)."""
    bad(e, "args.n_rays", -1)
    nulls(e, "args.packed_coarse", "args.rays", "args.weights_coarse", "args.feature_coarse", "args.depth_coarse", "args.packed_fine", "args.weights_fine",
          "args.feature_fine", "args.depth_fine")
    bad(e, "args.rng_flags", 8, 8 | 1)
    if pair:
        bad(e, "args.rng_flags", 1, 2, 4, 7)
        for k in ("z_coarse_out", "noise_coarse_out", "noise_fine_out"):
            case(e, "%s on a pair core" % k, **{"args." + k: P})
    else:
        case(e, "jitter with z_coarse", **{"args.rng_flags": 1, "args.z_coarse": P})
        case(e, "jitter and u with z_coarse", **{"args.rng_flags": 3, "args.z_coarse": P, "args.z_coarse_out": P})
        case(e, "u with u", **{"args.rng_flags": 2, "args.u": P})
        case(e, "noise with noise_coarse", **{"args.rng_flags": 4, "args.noise_coarse": P})
        case(e, "noise with noise_fine", **{"args.rng_flags": 7, "args.noise_fine": P})


for e, pair in (("crnerf_render_rays_f32", False), ("crnerf_render_rays_bf16", True), ("crnerf_render_rays_f32x3", False), ("crnerf_render_rays_f32h2", False),
                ("crnerf_render_rays_f32x3_repair", False), ("crnerf_render_rays_f16", True)):
    entry(e, args=RENDER, stream=None)
    nulls(e, "args")
    render_checks(e, pair)
    noop(e, "n_rays=0", **{"args.n_rays": 0})
for e, pair in (("crnerf_render_rays_train_f32", False), ("crnerf_render_rays_train_bf16", True), ("crnerf_render_rays_train_f32x3", False),
                ("crnerf_render_rays_train_f32h2", False), ("crnerf_render_rays_train_f32x3_repair", False)):
    entry(e, args=RENDER_TRAIN, acts_coarse=P, acts_fine=P, raw_coarse=P, raw_fine=P, stream=None)
    nulls(e, "args", "acts_coarse", "raw_coarse", "acts_fine", "raw_fine", "args.z_fine")
    case(e, "the saved state before the render checks", acts_coarse=None, **{"args.n_rays": -1, "args.rays": None})
    render_checks(e, pair)
    noop(e, "n_rays=0", **{"args.n_rays": 0})
e = entry("crnerf_render_rays_bf16_fine", args=RENDER_FINE, stream=None)
nulls(e, "args", "args.packed_fine", "args.rays", "args.weights_coarse", "args.weights_fine", "args.feature_fine", "args.depth_fine")
bad(e, "args.n_rays", -1)
bad(e, "args.n_importance", 0, -1)
bad(e, "args.rng_flags", 1, 8)
for k in ("z_coarse_out", "noise_coarse_out", "noise_fine_out"):
    case(e, k, **{"args." + k: P})
noop(e, "n_rays=0", **{"args.n_rays": 0})
e = entry("crnerf_render_rays_lean_f32", args=RENDER_LEAN, stream=None)
nulls(e, "args", "args.packed_coarse", "args.packed_fine", "args.rays", "args.feature_fine", "args.depth_fine")
bad(e, "args.n_rays", -1)
bad(e, "args.n_importance", 0, 257)
bad(e, "args.n_samples", 2, 257)
bad(e, "args.rng_flags", 1, 8)
for k in ("z_coarse_out", "noise_coarse_out", "noise_fine_out"):
    case(e, k, **{"args." + k: P})
noop(e, "n_rays=0", **{"args.n_rays": 0})


# ---- the render entries of include/crnerf_lean.h and include/crnerf_lean_composite.h, check by check in abi.hip's order
def companion_checks(e, ni, ns, required):
    """ni, ns: (refused below, lowest accepted, highest accepted, refused above) of n_importance and n_samples.  A bound's accepting side shows in the
    NEXT check answering: n_samples behind n_importance, the first required pointer behind n_samples."""
    nulls(e, "args")
    noop(e, "n_rays=0", **{"args.n_rays": 0})
    bad(e, "args.n_rays", -1)
    bad(e, "args.n_importance", ni[0], ni[3])
    for v in sorted({ni[1], ni[2]}):
        case(e, "n_importance=%d passes, n_samples answers" % v, **{"args.n_importance": v, "args.n_samples": ns[3]})
    bad(e, "args.n_samples", ns[0], ns[3])
    for v in (ns[1], ns[2]):
        case(e, "n_samples=%d passes, %s answers" % (v, required[0]), **{"args.n_samples": v, "args." + required[0]: None})
    nulls(e, *["args." + k for k in required])
    bad(e, "args.rng_flags", 1, 8)
    for k in ("z_coarse_out", "noise_coarse_out", "noise_fine_out"):
        case(e, k, **{"args." + k: P})


for e in ("crnerf_render_rays_lean_bf16", "crnerf_render_rays_lean_f16"):
    entry(e, args=RENDER_LEAN, stream=None)
    companion_checks(e, (0, 1, 256, 257), (2, 3, 256, 257), ("packed_coarse", "packed_fine", "rays", "feature_fine", "depth_fine"))
RENDER_CW = S("RenderArgs", packed_coarse=P, rays=P, n_rays=1, n_samples=2, n_importance=0, weights_coarse=P)
for e in ("crnerf_render_coarse_weights_f32h2", "crnerf_render_coarse_weights_f32x3", "crnerf_render_coarse_weights_f32x3_repair",
          "crnerf_render_coarse_weights_f16"):
    entry(e, args=RENDER_CW, stream=None)
    companion_checks(e, (-1, 0, 0, 1), (1, 2, 256, 257), ("packed_coarse", "rays", "weights_coarse"))
RENDER_LEAN_FINE = S("RenderArgs", packed_fine=P, rays=P, n_rays=1, n_samples=3, n_importance=1, weights_coarse=P, feature_fine=P, depth_fine=P)
e = entry("crnerf_render_rays_lean_bf16_fine", args=RENDER_LEAN_FINE, stream=None)
companion_checks(e, (0, 1, 256, 257), (2, 3, 256, 257), ("packed_fine", "rays", "weights_coarse", "feature_fine", "depth_fine"))
# the launch layer behind them: the one-workgroup-per-quad grid of the repair launch
case("crnerf_render_coarse_weights_f32x3_repair", "more ray quads than a launch", **{"args.n_rays": 2 ** 34, "args.n_samples": 4})


# ---- the launch layer behind abi.hip (csrc/launch.h and the launchers' own refusals): every one fires before anything is launched
def sample_count_checks(e, skip=()):
    """What launch.h's check_sample_counts refuses, in the order it checks."""
    for ns, ni in ((1, None), (257, None), (64, 257), (64, -1), (2, 1)):
        label = "n_samples=%d" % ns + ("" if ni is None else ", n_importance=%d" % ni)
        if label not in skip:
            case(e, label, **{"args.n_samples": ns}, **({} if ni is None else {"args.n_importance": ni}))


for e in ("crnerf_render_rays_f32", "crnerf_render_rays_bf16", "crnerf_render_rays_f32x3", "crnerf_render_rays_f32h2", "crnerf_render_rays_f32x3_repair",
          "crnerf_render_rays_f16", "crnerf_render_rays_train_f32", "crnerf_render_rays_train_bf16", "crnerf_render_rays_train_f32x3",
          "crnerf_render_rays_train_f32h2", "crnerf_render_rays_train_f32x3_repair"):
    sample_count_checks(e)
sample_count_checks("crnerf_render_rays_bf16_fine", skip=("n_samples=64, n_importance=-1",))      # abi.hip refuses that one itself (above)
# the saved rows' 32-bit offsets (not crnerf_render_rays_train_f32: its launcher has no such limit, the call would go on to a launch)
for e in ("crnerf_render_rays_train_bf16", "crnerf_render_rays_train_f32x3", "crnerf_render_rays_train_f32h2", "crnerf_render_rays_train_f32x3_repair"):
    case(e, "more sample points than 32-bit row offsets reach", **{"args.n_rays": 2 ** 20, "args.n_samples": 8, "args.n_importance": 8})
# the repair launches: one workgroup per ray quad / per 128 points
case("crnerf_render_rays_f32x3_repair", "more ray quads than a launch", **{"args.n_rays": 2 ** 34, "args.n_samples": 4, "args.n_importance": 0})
case("crnerf_mlp_forward_f32x3_repair", "more point groups than a launch", n=2 ** 39)

# ---- rays, encoder
e = entry("crnerf_ray_directions_f32", H=1, W=1, fx=1.0, fy=1.0, cx=0.0, cy=0.0, directions=P, stream=None)
nulls(e, "directions")
e = entry("crnerf_rays_from_directions_f32", directions=P, c2w_host=P, n=1, rays_o=P, rays_d=P, stream=None)
nulls(e, "directions", "c2w_host", "rays_o", "rays_d")
noop(e, "n=0", n=0)
e = entry("crnerf_generate_rays_f32", intrinsics_host=P, c2w_host=P, H=1, W=1, near=0.0, far=1.0, rays=P, stream=None)
nulls(e, "intrinsics_host", "c2w_host", "rays")
e = entry("crnerf_encoder_forward_f32", image=P, H=8, W=8, weights=L, workspace=P, out=P, stream=None)
nulls(e, "image", "weights", "workspace", "out")
holes(e, "weights", ENC)
e = entry("crnerf_encoder_forward_train_f32", image=P, H=8, W=8, weights=L, saved=P, out=P, stream=None)
nulls(e, "image", "weights", "saved", "out")
holes(e, "weights", ENC)
e = entry("crnerf_encoder_forward_train_band_f32", image_rows=P, H=8, W=8, H_image=8, row0=0, o0=0, o1=1, weights=L, saved=P, out=P, stream=None)
nulls(e, "image_rows", "weights", "saved", "out")
holes(e, "weights", ENC)
e = entry("crnerf_encoder_backward_band_f32", H=8, W=8, H_image=8, row0=0, o0=0, o1=1, weights=L, saved=P, out=P, d_out=P, scratch=P, grads=L, d_image_rows=None,
          stream=None)
nulls(e, "weights", "saved", "out", "d_out", "scratch", "grads")
bad(e, "H", 7)
bad(e, "W", 7)
holes(e, "weights", ENC)
holes(e, "grads", ENC)
e = entry("crnerf_encoder_backward_f32", H=8, W=8, weights=L, saved=P, out=P, d_out=P, scratch=P, grads=L, d_image=None, stream=None)
nulls(e, "weights", "saved", "out", "d_out", "scratch", "grads")
bad(e, "H", 7)
bad(e, "W", 7)
holes(e, "weights", ENC)
holes(e, "grads", ENC)

# ---- the cross-ray decoder
e = entry("crnerf_crossray_chansum_f32", x=P, HW=1, sum64=P, workspace=P, stream=None)
nulls(e, "x", "sum64", "workspace")
e = entry("crnerf_crossray_gram_f32", x=P, HW=1, mean64=P, cnn=L, gram_sum=P, workspace=P, stream=None)
nulls(e, "x", "mean64", "cnn", "gram_sum", "workspace")
holes(e, "cnn", 6)
e = entry("crnerf_crossray_matrix_f32", gram_sum=P, count=1.0, fc_w=P, fc_b=P, out=P, stream=None)
nulls(e, "gram_sum", "fc_w", "fc_b", "out")
e = entry("crnerf_crossray_fold_f32", s_matrix=P, c_matrix=P, c_mean64=P, s_mean64=P, lin=L, affine=P, stream=None)
nulls(e, "lin", "affine", "c_matrix", "c_mean64", "s_mean64")
holes(e, "lin", 6)
case(e, "a list entry before the matrices", c_matrix=None, **{"lin[3]": None})
e = entry("crnerf_crossray_apply_f32", x=P, HW=1, affine=P, rgb=P, plane_stride=1, stream=None)
nulls(e, "x", "affine", "rgb")
noop(e, "HW=0", HW=0)
e = entry("crnerf_crossray_decode_f32", content=P, HW=1, style=P, HWs=1, weights=L, workspace=P, rgb=P, plane_stride=1, stream=None)
nulls(e, "content", "weights", "workspace", "rgb")
bad(e, "HW", -1)
bad(e, "HWs", -1)
holes(e, "weights", DEC)
noop(e, "HW=0", HW=0)
e = entry("crnerf_crossray_decode_sharded_f32", content=P, HW_local=1, style=P, HWs=1, weights=L, phase=0, xchg=P, count_global=1.0, workspace=P, rgb=P,
          plane_stride=1, stream=None)
nulls(e, "style", "weights", "xchg", "workspace", "content")
bad(e, "HW_local", -1)
bad(e, "phase", -1, 3)
case(e, "rgb in phase 2", phase=2, rgb=None)
holes(e, "weights", DEC)
case(e, "no pixels: content is not read", HW_local=0, content=None, **{"weights[7]": None})
e = entry("crnerf_crossray_decode_backward_f32", content=P, HW=1, style=P, HWs=1, weights=L, d_rgb=P, d_plane_stride=1, workspace=P, d_content=P, d_style=P, grads=L,
          stream=None)
nulls(e, "content", "style", "weights", "d_rgb", "workspace", "d_content", "d_style", "grads")
bad(e, "HW", 0, -1)
bad(e, "HWs", 0)
holes(e, "weights", DEC)
holes(e, "grads", DEC)
e = entry("crnerf_crossray_decode_backward_sharded_f32", content=P, HW=1, style=P, HWs=1, weights=L, d_rgb=P, d_plane_stride=1, workspace=P, d_content=P, d_style=P,
          grads=L, phase=0, fwd_xchg=P, count_global=1.0, xb=P, stream=None)
nulls(e, "content", "style", "weights", "d_rgb", "workspace", "d_content", "d_style", "grads", "fwd_xchg", "xb")
bad(e, "HW", 0)
bad(e, "HWs", 0, -1)
bad(e, "phase", -1, 3)
holes(e, "weights", DEC)
holes(e, "grads", DEC)
e = entry("crnerf_decoder_content_backward_f32", content=P, HW=1, rgb_w=P, rgb=P, rgb_plane_stride=1, d_rgb=P, d_plane_stride=1, workspace=P, d_content=P, d_w=P,
          d_b=P, stream=None)
nulls(e, "content", "rgb_w", "rgb", "d_rgb", "workspace", "d_content", "d_w", "d_b")
bad(e, "HW", -1)
noop(e, "HW=0", HW=0)

# ---- loss, batch, optimiser
e = entry("crnerf_loss_f32", args=LOSS, losses=P, workspace=P, stream=None)
nulls(e, "args", "losses", "workspace", "args.rgb_coarse", "args.targets")
bad(e, "args.n_rays", 0, -1)
case(e, "rec without random", **{"args.a_embedded_random_rec": P})
case(e, "content_wo alone", **{"args.content_wo": P})
case(e, "content_with alone", **{"args.content_with": P})
e = entry("crnerf_loss_backward_f32", args=LOSS, upstream=P, grads=S("LossGrads"), stream=None)
nulls(e, "args", "upstream", "grads", "args.rgb_coarse", "args.targets")
bad(e, "args.n_rays", 0)
e = entry("crnerf_grid_sample_batch_f32", args=BATCH, stream=None)
nulls(e, "args", *["args." + k for k in ("all_rays", "all_rgbs", "w_lin", "h_lin", "rays", "ts", "rgbs", "rgb_idx", "uv_sample")])
bad(e, "args.img_w", 0)
bad(e, "args.img_h", 0)
bad(e, "args.ray_stride", 8)
noop(e, "side=0", **{"args.side": 0})
e = entry("crnerf_adam_step_f32", params=P, exp_avg=P, exp_avg_sq=P, blocks=P, n_blocks=1, grads=L, n_tensors=1, step_size=1.0, beta1=0.9, beta2=0.999, eps=0.0,
          weight_decay=0.0, bias_correction2_sqrt=1.0, stream=None)
nulls(e, "params", "exp_avg", "exp_avg_sq", "blocks", "grads")
bad(e, "n_tensors", 0, 449)
bad(e, "bias_correction2_sqrt", 0.0, -1.0)
bad(e, "eps", -1.0)
noop(e, "n_blocks=0", n_blocks=0)

# ---- metrics, image preparation, scene bounds
e = entry("crnerf_image_metrics_f32", args=METRICS, out2=P, ssim_map=None, workspace=P, stream=None)
nulls(e, "args", "out2", "workspace", "args.pred", "args.gt")
for k in ("channels", "width", "height", "w", "h"):
    bad(e, "args." + k, 0)
for k in ("w", "h"):
    bad(e, "args." + k, 1)
for k in ("x0", "y0"):
    bad(e, "args." + k, -1, 1)
case(e, "more tiles than a launch", **{"args.channels": 3, "args.width": 1 << 20, "args.height": 1 << 20, "args.w": 1 << 20, "args.h": 1 << 20})
e = entry("crnerf_lpips_f32", args=LPIPS, out6=P, features=L, workspace=P, stream=None)
nulls(e, "args", "out6", "workspace", "args.pred", "args.gt", "args.shift", "args.scale")
nulls(e, "args.conv_w[0]", "args.conv_w[4]", "args.conv_b[0]", "args.conv_b[4]", "args.lin[0]", "args.lin[4]")
holes(e, "features", 10)
for k in ("width", "height", "w", "h"):
    bad(e, "args." + k, 0)
for k in ("w", "h"):
    bad(e, "args." + k, 30)
for k in ("x0", "y0"):
    bad(e, "args." + k, -1, 1)
case(e, "more blocks than a launch", **{"args.width": 1 << 20, "args.height": 1 << 20, "args.w": 1 << 20, "args.h": 1 << 20})
case(e, "conv_w[1] off 16 bytes", **{"args.conv_w[1]": PTR + 8})
case(e, "conv_w[4] off 16 bytes", **{"args.conv_w[4]": PTR + 4})
e = entry("crnerf_lanczos_resize_u8", src=P, H=2, W=2, w=1, h=1, kx=P, bounds_x=P, ksize_x=13, ky=P, bounds_y=P, ksize_y=13, out_mode=0, dst=P, workspace=P,
          stream=None)
nulls(e, "src", "dst", "kx", "bounds_x", "ky", "bounds_y", "workspace")
for k in ("H", "W", "w", "h"):
    bad(e, k, 0)
bad(e, "out_mode", -1, 4)
bad(e, "ksize_x", 12)
bad(e, "ksize_y", 12)
case(e, "kx off 16 bytes", kx=PTR + 8)
case(e, "over 2^31 bytes", H=30000, W=30000, w=30000, h=30000)
e = entry("crnerf_scene_bounds_f64", xyz=P, n_points=1, w2c_row2=P, n_images=1, q_lo=0.1, q_hi=99.9, nears=P, fars=P, counts=P, workspace=None, stream=None)
nulls(e, "xyz", "w2c_row2", "nears", "fars", "counts")
bad(e, "n_images", 0)
bad(e, "n_points", -1)
bad(e, "q_lo", -1.0, 101.0, NAN, INF)
bad(e, "q_hi", -1.0, 101.0, NAN, -INF, 0.05)

# ---- the segmentation network's layers and chain
e = entry("crnerf_conv2d_f32", geom=GEOM, x=P, w=P, y=P, stream=None)
nulls(e, "geom", "x", "w", "y")
for k in ("cin", "cout", "H", "W", "k", "stride", "dil"):
    bad(e, "geom." + k, 0)
bad(e, "geom.pad", -1)
case(e, "depth-wise with cin != cout", **{"geom.depthwise": 1, "geom.cout": 2})
case(e, "empty output", **{"geom.k": 3})
e = entry("crnerf_conv2d_backward_f32", geom=GEOM, x=P, w=P, d_y=P, d_x=None, d_w=P, stream=None)
nulls(e, "geom", "x", "w", "d_y", "d_w")
bad(e, "geom.cin", 0)
case(e, "depth-wise with cin != cout", **{"geom.depthwise": 1, "geom.cin": 2})
case(e, "empty output", **{"geom.k": 2})
e = entry("crnerf_bn_prelu_f32", x=P, gamma=P, beta=P, alpha=P, mean=P, invstd=P, var_unbiased=None, y=P, C=1, HW=1, eps=1e-3, training=0, stream=None)
nulls(e, "x", "gamma", "beta", "alpha", "mean", "invstd", "y")
bad(e, "training", 1)
bad(e, "C", 0)
bad(e, "HW", 0, (1 << 30) + 1)
e = entry("crnerf_bn_prelu_train_f32", x=P, gamma=P, beta=P, alpha=P, mean=P, invstd=P, var_unbiased=P, y=P, running_mean=P, running_var=P, num_batches_tracked=None,
          momentum=0.1, C=1, HW=1, eps=1e-3, stream=None)
nulls(e, "x", "gamma", "beta", "alpha", "mean", "invstd", "y", "var_unbiased", "running_mean", "running_var")
bad(e, "C", 0)
bad(e, "HW", 0, (1 << 30) + 1)
bad(e, "momentum", -0.5, 1.5)
e = entry("crnerf_bn_prelu_backward_f32", x=P, gamma=P, beta=P, alpha=P, mean=P, invstd=P, d_y=P, d_x=P, d_gamma=P, d_beta=P, d_alpha=P, C=1, HW=1, training=1,
          stream=None)
nulls(e, "x", "gamma", "beta", "alpha", "mean", "invstd", "d_y", "d_x", "d_gamma", "d_beta", "d_alpha")
bad(e, "C", 0)
bad(e, "HW", 0, (1 << 30) + 1)
e = entry("crnerf_avgpool3s2_f32", inp=P, out=P, C=1, H=1, W=1, backward=0, stream=None)
nulls(e, "inp", "out")
for k in ("C", "H", "W"):
    bad(e, k, 0)
e = entry("crnerf_fglo_f32", x=P, w1=P, b1=P, w2=P, b2=P, stats=P, y=P, C=1, R=1, HW=1, stream=None)
nulls(e, "x", "w1", "b1", "w2", "b2", "stats", "y")
bad(e, "C", 0)
bad(e, "R", 0)
bad(e, "HW", 0, (1 << 22) + 1)
e = entry("crnerf_fglo_backward_f32", x=P, w1=P, w2=P, stats=P, d_y=P, scratch=P, d_x=P, d_w1=P, d_b1=P, d_w2=P, d_b2=P, C=1, R=1, HW=1, stream=None)
nulls(e, "x", "w1", "w2", "stats", "d_y", "scratch", "d_x", "d_w1", "d_b1", "d_w2", "d_b2")
bad(e, "C", 0, 257)
bad(e, "R", 0, 65)
bad(e, "HW", 0, (1 << 22) + 1)
e = entry("crnerf_bilinear_gather_f32", inp=P, h=1, w=1, Ho=1, Wo=1, idx=P, n=1, sigmoid=0, out=P, stream=None)
nulls(e, "inp", "out")
for k in ("h", "w", "Ho", "Wo"):
    bad(e, k, 0)
bad(e, "n", -1)
case(e, "no idx: n must be Ho*Wo", idx=None, n=2)
noop(e, "n=0", n=0)
e = entry("crnerf_bilinear_gather_backward_f32", out=None, d_out=P, h=1, w=1, Ho=1, Wo=1, idx=P, n=1, sigmoid=0, d_in=P, stream=None)
nulls(e, "d_in", "d_out")
for k in ("h", "w", "Ho", "Wo"):
    bad(e, k, 0)
bad(e, "n", -1)
bad(e, "sigmoid", 1)
case(e, "no idx: n must be Ho*Wo", idx=None, n=2)
case(e, "no idx, no points", idx=None, n=0, d_out=None)
e = entry("crnerf_cgnet_forward_train_f32", image=P, cin=1, H=1, W=1, params=L, running_mean=L, running_var=L, num_batches_tracked=None, momentum=0.1, eps=1e-3,
          saved=P, mask=P, stream=None)
nulls(e, "image", "saved", "mask", "running_mean", "running_var", "params")
bad(e, "cin", 0)
bad(e, "H", 0)
bad(e, "W", 0)
case(e, "over 2^24 pixels", H=4097, W=4097)
holes(e, "params", CG)
holes(e, "running_mean", BN)
holes(e, "running_var", BN)
bad(e, "eps", 0.0)
bad(e, "momentum", -0.5, 2.0)
e = entry("crnerf_cgnet_backward_f32", image=P, cin=1, H=1, W=1, params=L, saved=P, mask=P, d_mask=P, scratch=P, grads=L, stream=None)
nulls(e, "image", "saved", "mask", "d_mask", "scratch", "grads", "params")
bad(e, "cin", 0)
case(e, "over 2^24 pixels", H=4097, W=4097)
holes(e, "params", CG)
holes(e, "grads", CG)


def key(e, label):
    return "%s / %s" % (e, label)


def _struct(_lib, spec, overrides, all_null):
    obj = getattr(_lib, spec.name)()
    for f, v in ({} if all_null else spec.fields).items():
        _set_field(obj, f, v)
    for f, v in overrides.items():
        _set_field(obj, f, v)
    return obj


def _set_field(obj, f, v):
    v = PTR if v is P else v
    if "[" in f:
        name, i = f[:-1].split("[")
        getattr(obj, name)[int(i)] = v
    elif isinstance(getattr(obj, f), ctypes.Array):
        for i in range(len(getattr(obj, f))):
            getattr(obj, f)[i] = v
    else:
        setattr(obj, f, v)


def build_args(_lib, e, mut, is_noop):
    """The ctypes arguments of one case (and what they point to, to be kept alive across the call)."""
    base, argtypes = BASES[e], _lib.ALL_SIGNATURES[e][1]
    assert len(base) == len(argtypes), "%s: the base call has %d arguments, the signature table %d" % (e, len(base), len(argtypes))
    known = set(base)
    for m in mut:
        assert m.split(".")[0].split("[")[0] in known, "%s: %s is not an argument" % (e, m)
    args, alive = [], []
    for (name, v), ct in zip(base.items(), argtypes):
        if is_noop and (v is P or v is L):
            v = None
        if name in mut:
            v = mut[name]
        sub = {m[len(name) + 1:]: x for m, x in mut.items() if m.startswith(name + ".")}
        holes_ = {int(m[len(name) + 1:-1]): x for m, x in mut.items() if m.startswith(name + "[")}
        if isinstance(v, S):
            obj = _struct(_lib, v, sub, is_noop)
            alive.append(obj)
            v = ctypes.byref(obj)
        elif v is L:
            arr = (ctypes.c_void_p * LIST_LEN)(*([PTR] * LIST_LEN))
            for i, x in holes_.items():
                arr[i] = x
            alive.append(arr)
            v = ctypes.cast(arr, ct)
        elif v is P:
            v = PTR
        if isinstance(v, int) and issubclass(ct, ctypes._Pointer):      # a typed host pointer (`*_host`, a struct): the dummy address in its type
            v = ctypes.cast(ctypes.c_void_p(v), ct)
        args.append(v)
    return args, alive


def run_case(lib, _lib, e, mut, is_noop):
    """(code, text) of one case, behind the priming call."""
    assert getattr(lib, PRIME[0])(None, None) == -1
    args, alive = build_args(_lib, e, mut, is_noop)
    code = getattr(lib, e)(*args)
    del alive
    return int(code), lib.crnerf_last_error().decode()


def fixture_faults(table):
    """What must not be in a fixture: a case that reached HIP when it was recorded (it would launch on the dummy pointers on a GPU machine)."""
    noops = {key(e, label) for e, label, _, is_noop in CASES if is_noop}
    return ["%s: code %d" % (k, v["code"]) for k, v in table.items() if v["code"] == ERR_HIP or (v["code"] == 0) != (k in noops)]


def record():
    from crnerf_amd import _lib
    lib = _lib.load()
    table = {}
    for e, label, mut, is_noop in CASES:
        k = key(e, label)
        assert k not in table, "duplicate case %s" % k
        code, text = run_case(lib, _lib, e, mut, is_noop)
        table[k] = {"code": code, "message": text}
    return table


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=GOLDEN)
    a = ap.parse_args()
    table = record()
    faults = fixture_faults(table)
    if faults:
        raise SystemExit("refusing to record: these cases got through validation to a launch (or a no-op was refused):\n  " + "\n  ".join(faults))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(table, f, indent=0, sort_keys=True)
        f.write("\n")
    print("%s: %d cases of %d entry points, %d bytes, library %s" % (a.out, len(table), len({e for e, _, _, _ in CASES}), os.path.getsize(a.out),
                                                                      os.environ.get("CRNERF_LIB_PATH", "(shipped)")))

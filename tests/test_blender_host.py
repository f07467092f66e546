"""CPU-only side of the Blender dataset path: the numpy restatement of tests/_blender_cases.py against Pillow's and the
reference's recorded outputs (tests/golden/g19_blender.npz) and against Pillow live, the conditions those outputs must meet for the GPU
tests to mean something, perturbation_params against the reference's add_perturbation, include/crnerf_blender.h against
its table of _lib.HEADER_SIGNATURES, and every refusal of the entry points (no device is touched).  Every comparison is exact."""
import ctypes
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import _abi
import _blender_cases as B
from crnerf_amd import _lib
from crnerf_amd.datasets import blender

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = B.table_cases()


@pytest.fixture(scope="module")
def golden():
    return B.load_golden()


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_restatement_equals_pillows_recorded_output(golden, case):
    key, _, _, H, W, w, h = case
    a = B.case_input(case)
    assert np.array_equal(B.resize(a, (w, h)), golden["out_" + key])
    assert B.clip_count(a, (w, h)) == int(golden["clips"][[str(k) for k in golden["keys"]].index(key)])


def test_restatement_equals_pillow_live():
    Image = pytest.importorskip("PIL.Image")
    for case in CASES:
        key, _, _, H, W, w, h = case
        a = B.case_input(case)
        assert np.array_equal(B.resize(a, (w, h)), np.asarray(Image.fromarray(a).resize((w, h), Image.LANCZOS))), key


def test_identity_keeps_the_bytes_of_translucent_pixels(golden):
    case = next(c for c in CASES if c[0] == "identity_edges")
    a = B.case_input(case)
    assert np.array_equal(golden["out_identity_edges"], a)
    assert not np.array_equal(B.unpremultiply(B.premultiply(a))[0], a)          # the round trip Pillow's early copy() avoids is lossy here


@pytest.mark.parametrize("name", B.SHARES)
def test_blocks_cases_reach_all_three_unpremultiply_branches(golden, name):
    alpha = golden["out_%s_blocks" % name][..., 3]
    shares = [float((alpha == 0).mean()), float((alpha == 255).mean()), float(((alpha > 0) & (alpha < 255)).mean())]
    assert min(shares) >= 0.10, shares


def test_some_case_clips_at_255(golden):
    clips = dict(zip((str(k) for k in golden["keys"]), (int(c) for c in golden["clips"])))
    assert any(clips[name + "_blocks"] > 0 for name in B.SHARES), clips


@pytest.mark.parametrize("seed", B.PERTURB_SEEDS)
@pytest.mark.parametrize("pset", B.PERTURB_SETS, ids=["_".join(p) for p in B.PERTURB_SETS])
def test_perturbation_params_paint_what_the_reference_draws(golden, seed, pset):
    rects, colors, lut = blender.perturbation_params(list(pset), seed)
    assert rects.dtype == np.int32 and colors.dtype == np.uint8 and rects.shape == ((10, 4) if "occ" in pset else (0, 4))
    assert (lut is None) == ("color" not in pset)
    got = B.resize(B.perturb(B.frame(0), rects, colors, lut), B.IMG_WH)
    assert np.array_equal(got, golden["pert_%d_%s" % (seed, "_".join(pset))])


def test_colour_table_is_the_float64_expression_and_the_global_state_is_the_references():
    for seed in range(1, 21):
        _, _, lut = blender.perturbation_params(["occ", "color"], seed)
        state = np.random.get_state()
        np.random.seed(seed)
        s = np.random.uniform(0.8, 1.2, size=3)
        b = np.random.uniform(-0.2, 0.2, size=3)
        after = np.random.get_state()
        assert lut.dtype == np.uint8 and lut.shape == (3, 256) and np.array_equal(lut, B.color_table(s, b)), seed
        assert state[0] == after[0] and np.array_equal(state[1], after[1]) and state[2:] == after[2:]     # where add_perturbation leaves it
        # alpha passes (a / 255.0 * 255).astype(uint8) unchanged
    a = np.arange(256)
    assert np.array_equal((255 * (a / 255.0)).astype(np.uint8), a)
    # 'occ' alone ends on the last rectangle's colour draw
    blender.perturbation_params(["occ"], 3)
    state = np.random.get_state()
    np.random.seed(39)
    np.random.choice(range(256), 3)
    assert np.array_equal(state[1], np.random.get_state()[1]) and state[2] == np.random.get_state()[2]
    with pytest.raises(ValueError, match="Only"):
        blender.perturbation_params(["blur"], 1)


def test_intrinsics():
    K = blender.intrinsics(B.CAMERA_ANGLE_X, 40, 40)
    focal = 0.5 * 800 / np.tan(0.5 * B.CAMERA_ANGLE_X)
    focal *= 40 / 800
    assert K.dtype == np.float64 and np.array_equal(K, np.array([[focal, 0, 20.0], [0, focal, 20.0], [0, 0, 1]]))


def test_companion_header_declares_what_the_binding_expects():
    _abi.check_header("crnerf_blender.h")
    protos = _abi.prototypes("crnerf_blender.h")
    assert len(protos) == 4 and not set(protos) & set(_lib.HEADER_SIGNATURES["crnerf.h"])
    text = _abi.header_text("crnerf_blender.h")
    for name, value in (("TILE_H", _lib.RGBA_TILE_H), ("TILE_W", _lib.RGBA_TILE_W), ("VBLOCK", _lib.RGBA_VBLOCK), ("MAX_RECTS", _lib.RGBA_MAX_RECTS)):
        assert re.search(r"#define CRNERF_RGBA_%s %d\b" % (name, value), text), name
    for name, value in _lib.RGBA_OUT.items():
        assert re.search(r"#define CRNERF_RGBA_OUT_%s %d\b" % (name.upper(), value), text), name
    # the struct's fields, in order
    assert [f for _, f, _ in _abi.struct_fields("crnerf_rgba_prepare_args")] == [f[0] for f in _lib.RgbaPrepareArgs._fields_]


def ksize(a, b):
    return int(math.ceil(3.0 * max(a / b, 1.0))) * 2 + 1


FAKE = 0x10000      # a non-NULL, 16-byte aligned address no refusal path reads


def prepare_args(**kw):
    """A call that would pass every check (40 x 60 -> 20 x 30, both passes), with the given fields replaced."""
    a = _lib.RgbaPrepareArgs()
    a.src, a.H, a.W, a.w, a.h = FAKE, 40, 60, 30, 20
    a.kx = a.bounds_x = a.ky = a.bounds_y = FAKE
    a.n_rects, a.out_mode = 0, 0
    a.dst = a.workspace = FAKE
    for k, v in kw.items():
        setattr(a, k, v)
    if "ksize_x" not in kw:
        a.ksize_x = ksize(a.W, a.w) if a.w != a.W and a.w > 0 else 0
    if "ksize_y" not in kw:
        a.ksize_y = ksize(a.H, a.h) if a.h != a.H and a.h > 0 else 0
    return a


RECTS_OK = (ctypes.c_int32 * 8)(0, 0, 3, 3, 2, 2, 2, 2)
RECTS_X = (ctypes.c_int32 * 8)(0, 0, 3, 3, 5, 2, 4, 2)
RECTS_Y = (ctypes.c_int32 * 8)(0, 0, 3, 3, 2, 2, 2, 1)
COLORS = (ctypes.c_uint8 * 6)(1, 2, 3, 4, 5, 6)
addr = ctypes.addressof
NULL, SHAPE, CONFIG = -1, -2, -3
REFUSALS = [
    ("src", dict(src=None), NULL), ("dst", dict(dst=None), NULL),
    ("H0", dict(H=0), SHAPE), ("W0", dict(W=0), SHAPE), ("w0", dict(w=0), SHAPE), ("h_negative", dict(h=-1), SHAPE),
    ("mode4", dict(out_mode=4), CONFIG), ("mode_negative", dict(out_mode=-1), CONFIG),
    ("kx", dict(kx=None), NULL), ("bounds_x", dict(bounds_x=None), NULL), ("ksize_x", dict(ksize_x=ksize(60, 30) + 2), CONFIG),
    ("kx_misaligned", dict(kx=FAKE + 4), SHAPE),
    ("ky", dict(ky=None), NULL), ("bounds_y", dict(bounds_y=None), NULL), ("ksize_y", dict(ksize_y=ksize(40, 20) - 2), CONFIG),
    ("rects17", dict(n_rects=17, rects=addr(RECTS_OK), colors=addr(COLORS)), SHAPE), ("rects_negative", dict(n_rects=-1), SHAPE),
    ("rects_null", dict(n_rects=2, colors=addr(COLORS)), NULL), ("colors_null", dict(n_rects=2, rects=addr(RECTS_OK)), NULL),
    ("rect_x", dict(n_rects=2, rects=addr(RECTS_X), colors=addr(COLORS)), SHAPE),
    ("rect_y", dict(n_rects=2, rects=addr(RECTS_Y), colors=addr(COLORS)), SHAPE),
    ("src_misaligned", dict(src=FAKE + 2), SHAPE),
    ("workspace", dict(workspace=None), NULL),
    ("two_gib", dict(H=23171, W=23171, w=23171, h=23171), SHAPE),
    ("rows", dict(H=70000, W=2, w=2, h=65536), SHAPE),
    ("lds", dict(H=8, W=8000, w=100, h=8), SHAPE),
]


@pytest.mark.parametrize("name,fields,code", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_rgba_prepare_refuses(name, fields, code):
    lib = _lib.load()
    lib.crnerf_rgba_prepare_u8(None, None)                      # leaves "args is NULL" behind: the message below must be this call's
    assert lib.crnerf_rgba_prepare_u8(ctypes.byref(prepare_args(**fields)), None) == code
    msg = lib.crnerf_last_error()
    assert msg and b"args is NULL" not in msg


def test_rgba_prepare_refuses_null_args_and_sizes_the_workspace():
    lib = _lib.load()
    assert lib.crnerf_rgba_prepare_u8(None, None) == NULL and b"args is NULL" in lib.crnerf_last_error()
    assert lib.crnerf_rgba_prepare_workspace_bytes(40, 60, 30, 20) == 40 * 30 * 4
    assert lib.crnerf_rgba_prepare_workspace_bytes(40, 60, 60, 20) == 0          # vertical pass alone
    assert lib.crnerf_rgba_prepare_workspace_bytes(40, 60, 30, 40) == 0          # horizontal pass alone
    assert lib.crnerf_rgba_prepare_workspace_bytes(40, 60, 60, 40) == 0
    assert lib.crnerf_rgba_prepare_workspace_bytes(0, 60, 30, 20) == 0
    assert lib.crnerf_rgba_prepare_workspace_bytes(800, 800, 25, 25) == 800 * 25 * 4


def test_grid_sample_batch_round_refuses_like_its_twin():
    lib = _lib.load()
    for fn in (lib.crnerf_grid_sample_batch_round_f32, lib.crnerf_grid_sample_batch_f32):
        assert fn(None, None) == NULL and b"args is NULL" in lib.crnerf_last_error()
        a = _lib.BatchArgs()
        assert fn(ctypes.byref(a), None) == 0                   # side <= 0: nothing to do
        a.side = 4
        assert fn(ctypes.byref(a), None) == NULL and b"all_rays is NULL" in lib.crnerf_last_error()
        for k in ("all_rays", "all_rgbs", "w_lin", "h_lin", "rays", "ts", "rgbs", "rgb_idx", "uv_sample"):
            setattr(a, k, FAKE)
        a.ray_stride, a.img_w, a.img_h = 9, 0, 8
        assert fn(ctypes.byref(a), None) == SHAPE and lib.crnerf_last_error()
        a.img_w, a.ray_stride = 8, 8
        assert fn(ctypes.byref(a), None) == SHAPE and lib.crnerf_last_error()


def test_generate_rays_fmanorm_refuses_like_its_twin():
    lib = _lib.load()
    four, twelve = (ctypes.c_float * 4)(50, 50, 20, 20), (ctypes.c_float * 12)(*([0.0] * 12))
    for fn in (lib.crnerf_generate_rays_fmanorm_f32, lib.crnerf_generate_rays_f32):
        assert fn(None, twelve, 4, 4, 2.0, 6.0, FAKE, None) == NULL and b"intrinsics is NULL" in lib.crnerf_last_error()
        assert fn(four, None, 4, 4, 2.0, 6.0, FAKE, None) == NULL and b"c2w is NULL" in lib.crnerf_last_error()
        assert fn(four, twelve, 4, 4, 2.0, 6.0, None, None) == NULL and b"rays is NULL" in lib.crnerf_last_error()
        assert fn(four, twelve, 0, 4, 2.0, 6.0, FAKE, None) == SHAPE and b"empty image" in lib.crnerf_last_error()
        assert fn(four, twelve, 4, -1, 2.0, 6.0, FAKE, None) == SHAPE and b"empty image" in lib.crnerf_last_error()


def test_module_imports_without_the_library():
    code = ("import crnerf_amd.datasets.blender as b, crnerf_amd._lib as l; assert l._lib is None; "
            "r, c, t = b.perturbation_params(['occ', 'color'], 4); assert r.shape == (10, 4) and t.shape == (3, 256); "
            "b.intrinsics(0.69, 40, 40); assert l._lib is None; print('ok')")
    env = dict(os.environ, CRNERF_LIB_PATH=os.path.join(ROOT, "no_such_library.so"), PYTHONPATH=ROOT)
    out = subprocess.run([sys.executable, "-c", code], env=env, cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stderr

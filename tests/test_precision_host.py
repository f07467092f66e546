"""Every accepted spelling of a precision, and four that are not, through precision.resolve and the four setters that take one (no GPU needed)."""
import os
import re

import pytest
import torch

import crnerf_amd
from crnerf_amd import autograd, ops, precision
from crnerf_amd.models import nerf, rendering

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SPELLINGS = {
    "f32": ["f32", "fp32", "float32", torch.float32, None],
    "bf16": ["bf16", "bfloat16", torch.bfloat16],
    "f16": ["f16", "fp16", "float16", torch.float16],
    "f32x3": ["f32x3", "x3"],
    "f32h2": ["f32h2", "h2"],
    "auto": ["auto", "f32auto"],
    "bf16_hc": ["bf16_hc", "bf16+h2c"],
    "bf16_fc": ["bf16_fc", "bf16+f16c"],
}
COMPOSITE = ("bf16_hc", "bf16_fc")
REJECTS = ["garbage", "F32", torch.float64, 16]
ACCEPTED = [(s, name) for name, ss in SPELLINGS.items() for s in ss]
CASES = ACCEPTED + [(s, ValueError) for s in REJECTS]
IDS = [repr(s) for s, _ in CASES]


def check(setter, read, spelling, want):
    """setter(spelling) stores `want` (read() shows it), or raises when `want` is ValueError; the previous state comes back either way."""
    before = read()
    try:
        if want is ValueError:
            with pytest.raises(ValueError) as e:
                setter(spelling)
            assert repr(spelling) in str(e.value)
            assert read() == before                     # a refused value changes nothing
        else:
            setter(spelling)
            got = read()
            assert got == want and type(got) is type(want), (spelling, got, want)
    finally:
        restore(setter, before)
    assert read() == before


def restore(setter, before):
    slot = {autograd.set_wgrad_precision: autograd._WGRAD_BF16, autograd.set_training_forward_precision: autograd._TRAIN_FWD,
            autograd.set_training_precision: autograd._TRAIN_BF16}.get(setter)
    if slot is None:
        crnerf_amd.set_precision(before)
    else:
        slot[0] = before


def test_the_table_is_the_issue_s_table():
    assert precision.ALIASES == {s: name for s, name in ACCEPTED}
    assert set(precision.NAMES) == set(SPELLINGS) and set(precision.CORES) | {"auto"} | set(COMPOSITE) == set(SPELLINGS)


@pytest.mark.parametrize("spelling,name", CASES, ids=IDS)
def test_resolve(spelling, name):
    if name is ValueError:
        for composite in (False, True):
            with pytest.raises(ValueError) as e:
                precision.resolve(spelling, composite=composite)
            assert repr(spelling) in str(e.value)
            # the list of names in the message is the table's
            assert all(repr(n) in str(e.value) for n in SPELLINGS if composite or n not in COMPOSITE)
        return
    assert precision.resolve(spelling, composite=True) == name
    if name in COMPOSITE:
        with pytest.raises(ValueError) as e:
            precision.resolve(spelling)
        assert repr(spelling) in str(e.value) and "bf16_hc" not in str(e.value).replace(repr(spelling), "")
    else:
        assert precision.resolve(spelling) == name


@pytest.mark.parametrize("spelling,name", CASES, ids=IDS)
def test_set_precision(spelling, name):
    check(crnerf_amd.set_precision, crnerf_amd.get_precision, spelling, name)


@pytest.mark.parametrize("spelling,name", CASES, ids=IDS)
def test_set_training_forward_precision(spelling, name):
    want = None if spelling is None else name if name in ("f32", "f32x3", "f32h2", "auto") else ValueError
    check(autograd.set_training_forward_precision, lambda: autograd._TRAIN_FWD[0], spelling, want)


@pytest.mark.parametrize("spelling,name", CASES + [("bf16x3", "wgrad only"), ("f16x2", "wgrad only")], ids=IDS + ["'bf16x3'", "'f16x2'"])
def test_set_wgrad_precision(spelling, name):
    if spelling is None:
        want = None
    elif spelling in ("x3", "bf16x3"):
        want = 2
    elif spelling in ("h2", "f16x2"):
        want = 3
    elif name is ValueError or name in COMPOSITE:
        want = ValueError
    else:
        want = 1 if name == "bf16" else 0
    check(autograd.set_wgrad_precision, lambda: autograd._WGRAD_BF16[0], spelling, want)


@pytest.mark.parametrize("spelling,name", CASES, ids=IDS)
def test_set_training_precision(spelling, name):
    want = ValueError if (name is ValueError or name in COMPOSITE) else name == "bf16"
    check(autograd.set_training_precision, lambda: autograd._TRAIN_BF16[0], spelling, want)


def test_a_composite_mode_is_no_pack():
    class Args:
        nerf_out_dim = 64
    m = nerf.NeRF_sigma("coarse", Args(), in_channels_xyz=93, in_channels_dir=27)        # CPU parameters: a pack attempt would raise RuntimeError
    for spelling in SPELLINGS["bf16_hc"] + SPELLINGS["bf16_fc"] + REJECTS:
        with pytest.raises(ValueError):
            m.packed_weights(spelling)
        with torch.no_grad(), pytest.raises(ValueError):
            m(torch.zeros(4, 120), precision=spelling)
    assert m._packed is None


def test_no_is_helper_is_left():
    for mod in (crnerf_amd, ops, precision, autograd, nerf, rendering):
        assert [n for n in dir(mod) if n.startswith("_is_")] == [], mod.__name__
    pkg = os.path.join(ROOT, "cr-nerf-pytorch_amd")
    for d in (pkg, os.path.join(pkg, "models")):
        for f in sorted(os.listdir(d)):
            if f.endswith(".py"):
                with open(os.path.join(d, f)) as fh:      # a name of its own or one of ops': torch's t._is_view() and prose are none
                    assert not re.search(r"(?<![\w.])_is_\w+|ops\._is_\w+", fh.read()), f


def test_the_core_table_holds_exported_names():
    """Entry points by NAME (importing ops does not load the library), one record per core, every name one the library exports."""
    from crnerf_amd import _lib
    assert set(ops._CORES) == set(precision.CORES)
    for name, core in ops._CORES.items():
        entries = [e for e in core[:5] if e is not None]
        assert all(isinstance(e, str) for e in entries) and set(entries) <= set(_lib.EXPORTS), name
        assert (core.render_train is None) == (name == "f16") and (core.tag is ops.F16Pack) == (name == "f16")

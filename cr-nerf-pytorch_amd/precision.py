"""The precision names of the package and every spelling they are accepted under -- the one place a new mode is added.

CORES are the arithmetics a kernel family exists for (ops._CORES holds their entry points); "auto" is f32h2 with f32x3 as its safety net; the
COMPOSITE modes name a coarse / fine pairing of cores and exist for whole renders only (crnerf_amd.set_precision, render_rays_cross_ray)."""
import torch

CORES = ("f32", "bf16", "f16", "f32x3", "f32h2")
COMPOSITE = ("bf16_hc", "bf16_fc")

_SPELLINGS = {
    "f32": ("f32", "fp32", "float32", torch.float32, None),
    "bf16": ("bf16", "bfloat16", torch.bfloat16),
    "f16": ("f16", "fp16", "float16", torch.float16),
    "f32x3": ("f32x3", "x3"),
    "f32h2": ("f32h2", "h2"),
    "auto": ("auto", "f32auto"),
    "bf16_hc": ("bf16_hc", "bf16+h2c"),
    "bf16_fc": ("bf16_fc", "bf16+f16c"),
}
NAMES = tuple(_SPELLINGS)
ALIASES = {s: name for name, spellings in _SPELLINGS.items() for s in spellings}
_SINGLE = {s: name for s, name in ALIASES.items() if name not in COMPOSITE}


def resolve(precision, composite=False):
    """The canonical name of `precision`.  composite=False: the composite render modes are not accepted either.  ValueError for anything else."""
    try:
        return (ALIASES if composite else _SINGLE)[precision]
    except (KeyError, TypeError):       # TypeError: an unhashable value
        names = [n for n in NAMES if composite or n not in COMPOSITE]
        raise ValueError("crnerf_amd: precision must be %s or %r, got %r" % (", ".join(repr(n) for n in names[:-1]), names[-1], precision)) from None

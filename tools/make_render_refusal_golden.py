"""Records tests/golden/render_refusals.json: {case: [exception type name, full message]} of every refusal of ops.render_rays,
ops.render_coarse_weights and ops.render_rays_bf16_fine that fires before a device tensor is needed -- the mode exclusions, the precision refusals,
the pack checks and the refusal of CPU rays.  Run it on a machine WITHOUT a GPU, with the package whose answers are the contract (the fixture in the
tree was recorded before the three functions shared their pack resolution and their check-allocate-launch helper):

    python tools/make_render_refusal_golden.py [--out FILE]

ORDER is part of the contract: a case whose call breaks two rules records which one answers, and says so in its name ("A before B").  The packs are
CPU byte buffers of the size the library reports for their layout: nothing here is read on a device, and every case is refused before a launch.
tests/test_render_refusals_host.py imports its cases from here, so both always issue the same calls."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GOLDEN = os.path.join(ROOT, "tests", "golden", "render_refusals.json")
NC, NI = 8, 4
RNG = {"seed": 1, "jitter": True}


def _pack(name):
    """A CPU buffer with the byte size of a `name` pack (an F16Pack for "f16", an AutoPack for "auto")."""
    from crnerf_amd import _lib, ops
    if name == "auto":
        return ops.AutoPack(_pack("f32h2"), _pack("f32x3"))
    buf = torch.zeros(getattr(_lib.load(), ops._CORES[name].bytes)(), dtype=torch.uint8)
    return ops.F16Pack(buf) if name == "f16" else buf


def cases():
    """[(case name, function name, positional arguments, keyword arguments)]; built on call, because the packs need the library."""
    from crnerf_amd import ops
    pk = {n: _pack(n) for n in ("f32", "bf16", "f16", "f32x3", "f32h2", "auto")}
    short = torch.zeros(64, dtype=torch.uint8)
    no_h2 = ops.AutoPack(None, pk["f32x3"])
    rays = torch.zeros(4, 8)                     # on the CPU: the last refusal a call can reach without a device
    wc = torch.zeros(4, NC)
    out = []

    def rr(name, pc, pf, ni=NI, **kw):
        out.append(("render_rays / " + name, "render_rays", (pc, pf, rays, NC, ni), kw))

    def cw(name, pc, **kw):
        out.append(("render_coarse_weights / " + name, "render_coarse_weights", (pc, rays, NC), kw))

    def bf(name, pf, **kw):
        out.append(("render_rays_bf16_fine / " + name, "render_rays_bf16_fine", (pf, rays, wc, NC, NI), kw))

    f32 = (pk["f32"], pk["f32"])
    # ---- render_rays: the mode rules, in the order they are checked
    rr("an unknown precision", *f32, precision="f64")
    rr("a composite precision", *f32, precision="bf16_hc")
    rr("an unhashable precision", *f32, precision=[])
    rr("an unknown precision before lean with train", *f32, precision="f64", lean=True, train=True)
    rr("lean with train", *f32, lean=True, train=True)
    rr("lean with rng", *f32, lean=True, rng=RNG)
    rr("lean with train before the lean precisions", *f32, lean=True, train=True, precision="f32x3")
    for p in ("f32x3", "f32h2", "auto"):
        rr("lean under %s" % p, pk[p], pk[p], lean=True, precision=p)
    rr("lean under f32x3 before n_importance", pk["f32x3"], pk["f32x3"], ni=0, lean=True, precision="f32x3")
    rr("lean with n_importance 0", pk["f32"], None, ni=0, lean=True)
    rr("lean with n_importance 0 before repair_x3", pk["f16"], None, ni=0, lean=True, precision="f16", repair_x3=(pk["f32x3"], None))
    rr("lean with repair_x3", pk["f16"], pk["f16"], lean=True, precision="f16", repair_x3=(pk["f32x3"], pk["f32x3"]))
    rr("lean with launcher: the packs are next", short, pk["f32"], lean=True, launcher=True)
    for p in ("f32", "bf16", "f32x3", "f32h2", "auto"):
        rr("repair_x3 under %s" % p, pk[p], pk[p], precision=p, repair_x3=(pk["f32x3"], pk["f32x3"]))
    rr("repair_x3 under f32 before launcher with train", *f32, repair_x3=(pk["f32x3"], None), launcher=True, train=True)
    rr("f16 with train", pk["f16"], pk["f16"], precision="f16", train=True)
    rr("f16 with rng", pk["f16"], pk["f16"], precision="f16", rng=RNG)
    rr("f16 with train before launcher with train", pk["f16"], pk["f16"], precision="f16", train=True, launcher=True)
    rr("launcher with train", *f32, launcher=True, train=True)
    rr("launcher with train before the packs", short, short, launcher=True, train=True)
    # ---- render_rays: the packs
    rr("auto with a plain coarse pack", pk["f32h2"], pk["auto"], precision="auto")
    rr("auto with a plain fine pack", pk["auto"], pk["f32x3"], precision="auto")
    rr("auto with an F16Pack", pk["f16"], None, ni=0, precision="auto")
    rr("auto: the h2 pack of the wrong size", ops.AutoPack(short, pk["f32x3"]), None, ni=0, precision="auto")
    rr("auto without h2: the x3 pack of the wrong size", ops.AutoPack(None, short), None, ni=0, precision="auto")
    rr("auto, fine without h2: x3 throughout, the CPU rays answer", pk["auto"], no_h2, precision="auto")
    for p in ("f32", "bf16", "f32x3", "f32h2"):
        rr("%s: a coarse pack of the wrong size" % p, short, pk[p], precision=p)
        rr("%s: a fine pack of the wrong size" % p, pk[p], short, precision=p)
        rr("%s: an F16Pack" % p, pk["f16"], pk[p], precision=p)
    rr("f32: a bf16 pack", pk["bf16"], pk["bf16"])
    rr("f32: the coarse pack before the fine pack", short, pk["f16"])
    rr("f16: a plain coarse tensor", pk["bf16"], pk["f16"], precision="f16")
    rr("f16: a plain fine tensor", pk["f16"], pk["bf16"], precision="f16")
    rr("lean f16: a plain tensor", pk["bf16"], pk["f16"], precision="f16", lean=True)
    rr("a pack of the wrong size before CPU rays", short, None, ni=0)
    # ---- render_rays: CPU rays
    for p in ("f32", "bf16", "f16", "f32x3", "f32h2", "auto"):
        rr("%s: CPU rays" % p, pk[p], pk[p], precision=p)
    rr("lean: CPU rays", *f32, lean=True)
    rr("train: CPU rays", *f32, train=True)
    rr("rng under bf16: CPU rays come first", pk["bf16"], pk["bf16"], precision="bf16", rng=RNG)
    rr("f16 with repair_x3: CPU rays", pk["f16"], None, ni=0, precision="f16", repair_x3=(pk["f32x3"], None))

    # ---- render_coarse_weights
    cw("an unknown precision", pk["auto"], precision="f64")
    for p in ("f32", "bf16", "bf16_fc"):
        cw("precision %s" % p, pk["f32"], precision=p)
    cw("precision f32 before repair_x3", pk["f32"], precision="f32", repair_x3=pk["f32x3"])
    for p in ("f32h2", "f32x3", "auto"):
        cw("repair_x3 under %s" % p, pk[p], precision=p, repair_x3=pk["f32x3"])
    cw("repair_x3 under auto before the AutoPack check", pk["f32h2"], precision="auto", repair_x3=pk["f32x3"])
    cw("auto with a plain pack", pk["f32h2"])
    cw("auto with an F16Pack", pk["f16"])
    cw("auto with no pack", None)
    cw("auto: the h2 pack of the wrong size", ops.AutoPack(short, pk["f32x3"]))
    cw("auto: the x3 repair pack of the wrong size", ops.AutoPack(pk["f32h2"], short))
    cw("auto without h2: the x3 pack of the wrong size", ops.AutoPack(None, short))
    for p in ("f32h2", "f32x3"):
        cw("%s: a pack of the wrong size" % p, short, precision=p)
        cw("%s: an F16Pack" % p, pk["f16"], precision=p)
    cw("f16: a plain tensor", pk["bf16"], precision="f16")
    cw("f16: a repair pack of the wrong size", pk["f16"], precision="f16", repair_x3=short)
    cw("f16: an F16Pack as the repair pack", pk["f16"], precision="f16", repair_x3=pk["f16"])
    cw("f16: the pack before the repair pack", pk["bf16"], precision="f16", repair_x3=short)
    for p in ("f32h2", "f32x3", "auto", "f16"):
        cw("%s: CPU rays" % p, pk[p], precision=p)
    cw("auto without h2: CPU rays", no_h2)
    cw("f16 with repair_x3: CPU rays", pk["f16"], precision="f16", repair_x3=pk["f32x3"])

    # ---- render_rays_bf16_fine
    bf("a pack of the wrong size", short)
    bf("an f32 pack", pk["f32"])
    bf("an F16Pack", pk["f16"])
    bf("an F16Pack, lean", pk["f16"], lean=True)
    bf("CPU rays", pk["bf16"])
    bf("CPU rays, lean", pk["bf16"], lean=True)
    return out


def run_case(fn, args, kw):
    """[exception type name, message] of one case; a call that is not refused is an error of the case list."""
    from crnerf_amd import ops
    try:
        getattr(ops, fn)(*args, **kw)
    except Exception as e:  # noqa: BLE001 -- the type is what is recorded
        return [type(e).__name__, str(e)]
    raise AssertionError("%s(...) was not refused" % fn)


def record():
    table = {}
    for name, fn, args, kw in cases():
        assert name not in table, "duplicate case %s" % name
        table[name] = run_case(fn, args, kw)
    return table


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=GOLDEN)
    a = ap.parse_args()
    table = record()
    with open(a.out, "w") as f:
        json.dump(table, f, indent=0, sort_keys=True)
        f.write("\n")
    print("%s: %d cases, %d bytes" % (a.out, len(table), os.path.getsize(a.out)))

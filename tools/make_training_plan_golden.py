"""Records tests/golden/training_plan.json: what the training settings of crnerf_amd.autograd answer for a table of setter states and environments --
[get_training_forward_mode(), get_training_bf16(), get_wgrad_bf16(), get_wgrad_bf16(h2=True), get_training_recompute(), get_training_bf16_fused(),
the ray-chunk size fused_render_with_grad uses] per row.  Run it on a machine WITHOUT a GPU, with the package whose answers are the contract (the
fixture in the tree was recorded while six getters each read the environment themselves and the chunk size was an expression inside
fused_render_with_grad, which chunk_points() below restates):

    python tools/make_training_plan_golden.py [--out FILE]

Only the public setters and getters are used, so the same file records from any tree that has them.  The axes that do not interact are factored
instead of multiplied: the forward mode (setter x CRNERF_TRAIN_FWD x CRNERF_TRAIN_FWD_X3), the weight-gradient form (setter x the three CRNERF_WGRAD_*
variables alone, in pairs and together), bf16 and recompute (setter x environment each, recompute also x CRNERF_TRAIN_CHUNK_POINTS),
the three switches that choose a render's training path (bf16 and recompute, setter and environment, x CRNERF_TRAIN_BF16_UNFUSED), the spellings of
a flag for every flag, and a small cross of everything at once that shows the axes do not interact.
tests/test_training_plan_host.py imports its rows from here, so both always ask the same questions."""
import argparse
import contextlib
import itertools
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GOLDEN = os.path.join(ROOT, "tests", "golden", "training_plan.json")
FLAGS = ("CRNERF_TRAIN_FWD_X3", "CRNERF_WGRAD_F32", "CRNERF_WGRAD_BF16X3", "CRNERF_WGRAD_BF16", "CRNERF_TRAIN_BF16", "CRNERF_TRAIN_RECOMPUTE",
         "CRNERF_TRAIN_BF16_UNFUSED")
VARIABLES = FLAGS + ("CRNERF_TRAIN_FWD", "CRNERF_TRAIN_CHUNK_POINTS")
FORWARD_SETTER = (None, "f32", "f32x3", "f32h2", "auto")
WGRAD_SETTER = (None, "f32", "bf16", "bf16x3", "f16x2")
WGRAD_VARS = ("CRNERF_WGRAD_F32", "CRNERF_WGRAD_BF16X3", "CRNERF_WGRAD_BF16")


def rows():
    """[{"forward", "wgrad", "bf16", "recompute": what the four setters are given; "env": {variable: value}}]"""
    out = []

    def row(forward=None, wgrad=None, bf16=False, recompute=False, **env):
        r = {"forward": forward, "wgrad": wgrad, "bf16": bf16, "recompute": recompute, "env": env}
        if r not in out:                     # (the all-defaults row and a few others belong to several axes)
            out.append(r)

    for f, e, x3 in itertools.product(FORWARD_SETTER, (None, "x3", "h2", "fp32", "auto", "junk"), (None, "1")):
        row(forward=f, **{k: v for k, v in (("CRNERF_TRAIN_FWD", e), ("CRNERF_TRAIN_FWD_X3", x3)) if v is not None})
    for e in ("f32x3", "f32h2", "f32", "X3", "Auto"):                      # the other accepted spellings; the variable is lower-cased before it is read
        row(CRNERF_TRAIN_FWD=e)
    subsets = [s for n in range(4) for s in itertools.combinations(WGRAD_VARS, n)]
    for w, s in itertools.product(WGRAD_SETTER, subsets):
        row(wgrad=w, **{k: "1" for k in s})
    for f, w in itertools.product(FORWARD_SETTER, WGRAD_SETTER):            # (what "f16x2" means is the caller's h2 argument, not the forward mode)
        row(forward=f, wgrad=w)
    for b, e in itertools.product((False, True), (None, "", "0", "1")):
        row(bf16=b, **({} if e is None else {"CRNERF_TRAIN_BF16": e}))
    for r, e, c in itertools.product((False, True), (None, "", "0", "1"), (None, "12345")):
        row(recompute=r, **{k: v for k, v in (("CRNERF_TRAIN_RECOMPUTE", e), ("CRNERF_TRAIN_CHUNK_POINTS", c)) if v is not None})
    for b, eb, r, er, un in itertools.product((False, True), repeat=5):   # which training path a render takes: bf16, recompute and the un-fused switch
        row(bf16=b, recompute=r, **{k: "1" for k, on in (("CRNERF_TRAIN_BF16", eb), ("CRNERF_TRAIN_RECOMPUTE", er), ("CRNERF_TRAIN_BF16_UNFUSED", un)) if on})
    for name, v in itertools.product(FLAGS, ("", "0", "1", "yes")):
        row(**{name: v})
    for f, w, b, r, e in itertools.product((None, "f32h2"), (None, "bf16"), (False, True), (False, True), (False, True)):
        row(forward=f, wgrad=w, bf16=b, recompute=r, **({"CRNERF_TRAIN_FWD": "x3", "CRNERF_WGRAD_F32": "1", "CRNERF_TRAIN_BF16_UNFUSED": "1"} if e else {}))
    return out


def row_name(r):
    return json.dumps(r, sort_keys=True)


@contextlib.contextmanager
def applied(r):
    """The setters and the environment as row `r` says; both as they were afterwards (the setters at their defaults)."""
    from crnerf_amd import autograd as AG
    before = {k: os.environ.pop(k, None) for k in VARIABLES}
    os.environ.update(r["env"])
    try:
        AG.set_training_forward_precision(r["forward"])
        AG.set_wgrad_precision(r["wgrad"])
        AG.set_training_precision("bf16" if r["bf16"] else "f32")
        AG.set_training_recompute(r["recompute"])
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


def chunk_points():
    """The chunk size as fused_render_with_grad formed it when the fixture was recorded."""
    from crnerf_amd import autograd as AG
    return int(os.environ.get("CRNERF_TRAIN_CHUNK_POINTS", str(1 << (20 if AG.get_training_recompute() else 21))))


def getter_answers():
    from crnerf_amd import autograd as AG
    return [AG.get_training_forward_mode(), AG.get_training_bf16(), AG.get_wgrad_bf16(), AG.get_wgrad_bf16(h2=True), AG.get_training_recompute(),
            AG.get_training_bf16_fused(), chunk_points()]


def record():
    table = {}
    for r in rows():
        assert row_name(r) not in table, "duplicate row %s" % row_name(r)
        with applied(r):
            table[row_name(r)] = getter_answers()
    return table


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=GOLDEN)
    a = ap.parse_args()
    table = record()
    with open(a.out, "w") as f:
        json.dump(table, f, indent=0, sort_keys=True)
        f.write("\n")
    print("%s: %d rows, %d bytes" % (a.out, len(table), os.path.getsize(a.out)))

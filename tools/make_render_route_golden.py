"""Records tests/golden/render_routes.json: which launch models/rendering.py::render_rays_cross_ray gives a call, with which arguments -- the real
function on CPU tensors, its launch seams replaced by recorders, so no GPU and no libcrnerf_hip.so is needed:

    python tools/make_render_route_golden.py [--out FILE]          record (run it with the package whose answers are the contract)
    python tools/make_render_route_golden.py --show N              row N and its recorded outcome, spelled out
    python tools/make_render_route_golden.py --time                ms per 2,000 front-door calls against do-nothing seams (Python only)
    python tools/make_render_route_golden.py --ab PARENT_TREE      --time in child processes, the parent checkout (with a copy of this file in its
                                                                   tools/) against this tree, alternating P N, five of each

The seams (SEAMS below): the four ops.render_* launchers, rendering._render_unfused, autograd.fused_render_with_grad, NeRF_sigma.packed_weights (returns
a tag of (model.typ, precision)) and ops.in_kernel_rng.  Per row the outcome is the sequence of seam calls, every argument of each summarised (None and
scalars by value, a tensor by shape, dtype and SHA-256 -- the draws are CPU draws after torch.manual_seed(0), so this pins their order and shapes -- a
tensor another seam returned by where it came from, packs by their tag, the rng dict and the TrainPlan in full), and the returned dict as (key, which
seam tensor) pairs in order; or the exception's type and message.
rows(): the full product of precision x grad mode x pertubeCord x perturb x noise_std x N_samples x N_importance x lean x in-kernel RNG, and factored
in on a few rows of every path: the training plans, precision=None under set_precision, frozen models in grad mode, output_random / encode_random off,
rng_ray_offset, a view_dir tensor and use_disp.
The file stores every distinct argument value, result and outcome once ("values", "tails", "outcomes") and the rows, in rows() order, as indices;
expand() spells a row's outcome out again.  tests/test_render_route_host.py imports its rows and its replay from here."""
import argparse
import contextlib
import hashlib
import inspect
import itertools
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

GOLDEN = os.path.join(ROOT, "tests", "golden", "render_routes.json")
PRECISIONS = ("f32", "bf16", "f16", "f32x3", "f32h2", "auto", "bf16_hc", "bf16_fc")
N_SAMPLES, N_IMPORTANCE = (2, 3, 256, 257), (0, 1, 256, 257)
AXES = ("precision", "grad", "jitter", "perturb", "noise_std", "Nc", "Ni", "lean", "rng")
EXTRAS = {"plan": "default", "set_precision": False, "frozen": False, "output_random": True, "encode_random": True, "rng_ray_offset": 0,
          "view_dir": False, "use_disp": False}
PLANS = {"default": {}, "recompute": {"recompute": True}, "bf16": {"bf16": True}, "bf16+recompute": {"bf16": True, "recompute": True},
         "bf16+unfused": {"bf16": True, "env": {"CRNERF_TRAIN_BF16_UNFUSED": "1"}}}
SEAMS = ("render_rays", "render_rays_lean_x", "render_coarse_weights", "render_rays_bf16_fine", "_render_unfused", "fused_render_with_grad",
         "packed_weights")
COARSE_KEYS, FINE_KEYS = ("weights_coarse", "feature_coarse", "depth_coarse"), ("weights_fine", "feature_fine", "depth_fine")
R = 3


def rows():
    """[{axis or extra: value}]; the order is the order of the file's "rows"."""
    out = [dict(EXTRAS, **dict(zip(AXES, v)))
           for v in itertools.product(PRECISIONS, (False, True), (False, True), (0, 1), (0, 1), N_SAMPLES, N_IMPORTANCE, (False, True), (False, True))]
    counts = ((2, 0), (2, 1), (3, 1), (256, 256), (257, 1), (3, 257))
    for plan, jitter, perturb, (nc, ni), rng in itertools.product(list(PLANS)[1:], (False, True), (0, 1), counts, (False, True)):
        out.append(dict(EXTRAS, precision="f32", grad=True, jitter=jitter, perturb=perturb, noise_std=1, Nc=nc, Ni=ni, lean=False, rng=rng, plan=plan))
    extras = ({"set_precision": True}, {"frozen": True}, {"output_random": False}, {"encode_random": False}, {"rng_ray_offset": 7}, {"view_dir": True},
              {"use_disp": True})
    for extra, precision, grad, lean, (nc, ni), perturb in itertools.product(extras, ("f32", "auto", "bf16_hc", "bf16_fc"), (False, True), (False, True),
                                                                             ((3, 1), (3, 0), (257, 1)), (0, 1)):
        if "set_precision" in extra and precision != "f32":
            continue                                    # (one setting is enough to show the keyword's default is read)
        r = dict(EXTRAS, precision="bf16" if "set_precision" in extra else precision, grad=grad or "frozen" in extra, jitter=False, perturb=perturb,
                 noise_std=1, Nc=nc, Ni=ni, lean=lean, rng=True, **extra)
        if r not in out:
            out.append(r)
    return out


# ---- the seams

class PackTag:
    def __init__(self, typ, precision):
        self.tag = [typ, precision]


class Recorder:
    """What the seams were called with during one front-door call.  record=False (--time): the seams only return."""

    def __init__(self, record=True):
        self.record, self.calls, self.made, self.alive = record, [], {}, []
        if not record:
            import torch
            self.made = {k: torch.empty(0) for k in COARSE_KEYS + FINE_KEYS}

    def summarise(self, v):
        import torch
        if v is None or isinstance(v, (bool, int, float, str)):
            return v
        if isinstance(v, torch.Tensor):
            if id(v) in self.made:
                return {"from": self.made[id(v)]}
            return {"tensor": [list(v.shape), str(v.dtype).replace("torch.", ""), hashlib.sha256(v.detach().contiguous().numpy().tobytes()).hexdigest()]}
        if isinstance(v, PackTag):
            return {"pack": v.tag}
        if hasattr(v, "_fields"):
            return {"plan": dict(v._asdict())}
        if isinstance(v, (tuple, list)):
            return {"tuple": [self.summarise(x) for x in v]}
        if isinstance(v, dict):
            return {"rng": dict(v)}
        if hasattr(v, "typ"):
            return {"model": v.typ}
        raise TypeError("cannot summarise %r" % (v,))

    def returns(self, seam, arguments, keys):
        import torch
        self.calls.append([seam, {k: self.summarise(v) for k, v in arguments.items()}])
        out = {k: torch.empty(0) for k in keys}
        for k, t in out.items():
            self.made[id(t)] = "%d.%s" % (len(self.calls) - 1, k)
        self.alive.append(out)                  # (an id stays one tensor's for the whole call)
        return out


def _keys(seam, a):
    if seam == "render_coarse_weights":
        return COARSE_KEYS[:1]
    if seam == "render_rays_lean_x" or a.get("lean"):
        return FINE_KEYS[1:]
    if seam == "render_rays_bf16_fine":
        return FINE_KEYS
    return COARSE_KEYS + (FINE_KEYS if a.get("n_importance", a.get("Ni")) > 0 else ())


class Seams:
    """The package with its launch seams replaced; `state` is what they report to: {"rec": Recorder, "rng": what ops.in_kernel_rng() answers}."""

    def __init__(self):
        from crnerf_amd import autograd, ops
        from crnerf_amd.models import nerf, rendering
        self.rendering, self.nerf, self.state, self.saved, self.signatures = rendering, nerf, {"rec": None, "rng": True}, [], {}
        where = {"render_rays": ops, "render_rays_lean_x": ops, "render_coarse_weights": ops, "render_rays_bf16_fine": ops, "_render_unfused": rendering,
                 "fused_render_with_grad": autograd, "packed_weights": nerf.NeRF_sigma}
        for seam in SEAMS:
            self._replace(where[seam], seam)
        self.saved.append((ops, "in_kernel_rng", ops.in_kernel_rng))
        ops.in_kernel_rng = lambda: self.state["rng"]

    def _replace(self, owner, seam):
        real, state = getattr(owner, seam), self.state
        sig = self.signatures[seam] = inspect.signature(real)

        def stub(*a, **kw):
            if not state["rec"].record:                  # --time: every key any caller reads, nothing looked at
                return None if seam == "packed_weights" else dict(state["rec"].made)
            arguments = sig.bind(*a, **kw).arguments
            if seam == "packed_weights":
                tag = PackTag(arguments["self"].typ, arguments.get("precision", "f32"))
                state["rec"].calls.append([seam, {k: state["rec"].summarise(v) for k, v in arguments.items()}])
                return tag
            return state["rec"].returns(seam, arguments, _keys(seam, arguments))
        self.saved.append((owner, seam, real))
        setattr(owner, seam, stub)

    def restore(self):
        for owner, name, real in reversed(self.saved):
            setattr(owner, name, real)


@contextlib.contextmanager
def seams():
    s = Seams()
    try:
        yield s
    finally:
        s.restore()


# ---- one row

_fixed = {}


def _inputs(row):
    """(models, embeddings, rays, view_dir) of a row: CPU tensors, the same objects for every row that shares them."""
    import torch
    from crnerf_amd.models.nerf import NeRF_sigma, PosEmbedding

    class A:
        nerf_out_dim = 64
    if not _fixed:
        i = torch.arange(R, dtype=torch.float32)[:, None]
        d = torch.nn.functional.normalize(torch.cat([0.1 * i - 0.1, 0.05 * i, -torch.ones(R, 1)], 1), dim=1)
        _fixed["rays"] = torch.cat([0.01 * i.expand(R, 3), d, torch.full((R, 1), 2.0), torch.full((R, 1), 6.0)], 1)
        _fixed["view_dir"] = torch.nn.functional.normalize(d + 0.25, dim=1)
        _fixed["emb"] = {"xyz": PosEmbedding(14, 15), "dir": PosEmbedding(3, 4)}
        torch.manual_seed(1)
        for er in (False, True):
            _fixed[er] = {"coarse": NeRF_sigma("coarse", A(), in_channels_xyz=93, in_channels_dir=27),
                          "fine": NeRF_sigma("fine", A(), in_channels_xyz=93, in_channels_dir=27, encode_random=er)}
    models = _fixed[row["encode_random"]]
    for m in models.values():
        m.requires_grad_(not row["frozen"])
    return models, _fixed["emb"], _fixed["rays"], _fixed["view_dir"] if row["view_dir"] else None


def call(s, row):
    """The front-door call of `row` (its plan and precision setting in force), as the reference's callers make it: eleven positional arguments."""
    import torch
    models, emb, rays, view_dir = _inputs(row)

    class A:
        nerf_out_dim, pertubeCord = 64, row["jitter"]
    kw = {"args": A(), "lean": row["lean"]}
    if not row["set_precision"]:
        kw["precision"] = row["precision"]
    if view_dir is not None:
        kw["view_dir"] = view_dir
    if not row["output_random"]:
        kw["output_random"] = False
    if row["rng_ray_offset"]:
        kw["rng_ray_offset"] = row["rng_ray_offset"]
    s.state["rng"] = row["rng"]
    with (torch.enable_grad() if row["grad"] else torch.no_grad()):
        return s.rendering.render_rays_cross_ray(models, emb, rays, None, row["Nc"], row["use_disp"], row["perturb"], row["noise_std"], row["Ni"],
                                                 1024 * 32, False, **kw)


@contextlib.contextmanager
def settings(row):
    """The training plan and the precision setting of `row`; both as they were afterwards."""
    import crnerf_amd
    from make_training_plan_golden import applied
    before = crnerf_amd.get_precision()
    with applied(dict({"forward": None, "wgrad": None, "bf16": False, "recompute": False, "env": {}}, **PLANS[row["plan"]])):
        if row["set_precision"]:
            crnerf_amd.set_precision(row["precision"])
        try:
            yield
        finally:
            crnerf_amd.set_precision(before)


def replay(s, row):
    """The outcome of `row`, spelled out: {"calls": [[seam, {parameter: value}]], "returns": [[key, "<call>.<key>"]] | "raises": [type, message]}."""
    import torch
    rec = s.state["rec"] = Recorder()
    torch.manual_seed(0)
    with settings(row):
        try:
            res = call(s, row)
        except Exception as e:  # noqa: BLE001 -- the refusal is the outcome
            return {"calls": rec.calls, "raises": [type(e).__name__, str(e)]}
    return {"calls": rec.calls, "returns": [[k, rec.made[id(v)]] for k, v in res.items()]}


# ---- the file

def _intern(pool, v):
    return pool.setdefault(json.dumps(v, sort_keys=True), len(pool))


def record():
    values, tails, outcomes, index = {}, {}, {}, []
    with seams() as s:
        parameters = {seam: list(sig.parameters) for seam, sig in s.signatures.items()}
        for row in rows():
            o = replay(s, row)
            calls = []
            for seam, arguments in o["calls"]:           # per call: the seam and one value index per parameter, -1 where it was not passed
                vs = [_intern(values, arguments[p]) if p in arguments else -1 for p in parameters[seam]]
                while vs and vs[-1] == -1:
                    vs.pop()
                calls.append([SEAMS.index(seam)] + vs)
            tail = {k: o[k] for k in ("returns", "raises") if k in o}
            index.append(_intern(outcomes, [calls, _intern(tails, tail)]))
    return {"seams": [[seam, parameters[seam]] for seam in SEAMS], "values": [json.loads(k) for k in values], "tails": [json.loads(k) for k in tails],
            "outcomes": [json.loads(k) for k in outcomes], "rows": index}


def expand(table, i):
    """Row i's outcome as replay() gives it."""
    calls, tail = table["outcomes"][table["rows"][i]]
    out = {"calls": [[table["seams"][c[0]][0], {p: table["values"][v] for p, v in zip(table["seams"][c[0]][1], c[1:]) if v != -1}] for c in calls]}
    out.update(table["tails"][tail])
    return out


def canonical(outcome):
    return json.dumps(outcome, sort_keys=True)


# ---- --time / --ab

TIMED = {"inference": dict(EXTRAS, precision="f32", grad=False, jitter=False, perturb=0, noise_std=0, Nc=64, Ni=128, lean=False, rng=True),
         "grad": dict(EXTRAS, precision="f32", grad=True, jitter=False, perturb=1, noise_std=1, Nc=64, Ni=64, lean=False, rng=True)}
CALLS = 2000


def timed():
    """{"inference" | "grad": ms per CALLS front-door calls}: no draw tensors in either (the grad row draws in the kernel), so what is timed is the
    front door's own Python."""
    out = {}
    with seams() as s:
        for name, row in TIMED.items():
            with settings(row):
                for n in (200, CALLS):
                    s.state["rec"] = Recorder(record=False)
                    t0 = time.perf_counter()
                    for _ in range(n):
                        call(s, row)
                    out[name] = (time.perf_counter() - t0) * 1e3
    return out


def ab(parent_tree, reps=5):
    trees = {"P": os.path.join(os.path.abspath(parent_tree), "tools", os.path.basename(__file__)), "N": os.path.abspath(__file__)}
    got = {k: {name: [] for name in TIMED} for k in trees}
    print("render_rays_cross_ray against do-nothing seams, CPU only: parent commit (P) against this tree (N), child processes alternating P N, %d of each" % reps)
    for rep in range(reps):
        for k, tool in trees.items():
            t = json.loads(subprocess.run([sys.executable, tool, "--time"], check=True, stdout=subprocess.PIPE, text=True).stdout.splitlines()[-1])
            for name in TIMED:
                got[k][name].append(t[name])
            print("  %s rep %d: %s" % (k, rep, ", ".join("%s %.1f ms per %d calls (%.2f us per call)" % (n, t[n], CALLS, t[n] * 1e3 / CALLS) for n in TIMED)))
    for name in TIMED:
        p, n = got["P"][name], got["N"][name]
        spread, d = max(p) - min(p), statistics.median(n) - statistics.median(p)
        print("%s (ms per %d calls): parent median %.2f (min %.2f, max %.2f, spread %.2f), this tree median %.2f (min %.2f, max %.2f); this tree - parent = %+.2f: %s"
              % (name, CALLS, statistics.median(p), min(p), max(p), spread, statistics.median(n), min(n), max(n), d,
                 "within the parent's spread" if d <= spread else "BEYOND the parent's spread"))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=GOLDEN)
    ap.add_argument("--show", type=int)
    ap.add_argument("--time", action="store_true")
    ap.add_argument("--ab")
    a = ap.parse_args()
    if a.time:
        print(json.dumps(timed()))
    elif a.ab:
        ab(a.ab)
    elif a.show is not None:
        with open(GOLDEN) as f:
            print(json.dumps({"row": rows()[a.show], "outcome": expand(json.load(f), a.show)}, indent=1))
    else:
        t0 = time.perf_counter()
        table = record()
        with open(a.out, "w") as f:
            json.dump(table, f, separators=(",", ":"))
            f.write("\n")
        print("%s: %d rows, %d distinct outcomes, %d values, %d bytes, %.1f s"
              % (a.out, len(table["rows"]), len(table["outcomes"]), len(table["values"]), os.path.getsize(a.out), time.perf_counter() - t0))

"""The MLP weight gradients (csrc/mlp_train16.hip: wgrad_body<0|1|2|4>, wgrad_batch, the reduce kernels, launch_mlp_wgrads and its chunk plans)
held to the float64 reference BIT FOR BIT on operands for which every fp32 summation order is exact (tests/_wgrad_cases.py: construction,
certificate, reference, byte layout; tests/test_wgrad_exact_host.py: the certificate of every case used here, on the CPU).  The operands are
written straight into the saved state and the backward's scratch buffer, and ops.mlp_backward(phase="wgrad") runs the weight gradients alone --
in the four arithmetic modes (fp32 MFMA, single-piece bf16, bf16x3, f16x2) and both launch plans.  torch.equal leaves no room for a point dropped
or counted twice at a chunk edge, a clamped last row that leaks into a sum, a bias sum taken twice, a wrong column at M - 1 or N - 1 or a reduce
that skips a partial: each changes every sum by about one part in P, which no tolerance test sees.

The first test ties the helper's layout to the product; without it a wrong helper would make every other test meaningless.

f16x2 range words: the tests use the true maxima, zero, Inf (activation word) and words that UNDERSTATE (a stale word; the kernel's own range watch
must notice and fall back).  Words that OVERSTATE are outside the contract -- the data gradient only ever raises a zeroed word -- and are not tested.

MEASURED on an MI355X when these tests were written: all four modes return the float64 bits on every case, the 17- and 18-bit families included --
so v_mfma_f32_32x32x16_bf16 and v_mfma_f32_32x32x16_f16 keep every bit of a k = 16 dot product whose partial sums are fp32 numbers, like the fp32
MFMA does, and no mode's certificate had to be lowered.  The three large sizes take 0.1, 0.4 and 0.3 s (data, float64 reference, packing and the
four modes; the kernels themselves 10-20 ms), everything else well under 0.5 s a test.  Mutation check (scratch builds of mlp_train16.hip, one line
each; "oracle" = test_mlp_backward_vs_autograd_oracle and test_split_core_backward_vs_autograd_oracle of test_gpu_parity.py):
  `pt < p1` -> `pt <= p1` in wgrad_partial_tiles' fetch16             red here (97 tests), oracle green
  `< p1` -> `<= p1` in the single-piece bf16 take16                    red here (44), oracle green
  `u < 8` -> `u < 7` in the reduce (every eighth partial skipped)      red here (38), oracle green
  `&&` -> `||` in the full-tile f16x2 range watch                      red here (10: the fabricated-word tests), oracle green
  the reduce starting at partial 1                                     red here (157) and in the oracle (it drops a whole chunk)
  `grads[8] + XYZ_DIM - 1`                                             red here (186) and in the oracle
  `c < j.M` -> `c <= j.M` in wgrad_partial_tiles                       caught by NEITHER, and cannot be: row M of a tile is masked again at
                                                                       the store (`m < j.M`) and at the bias store, so the slip changes no output
"""
import time

import numpy as np
import pytest
import torch

import _wgrad_cases as C

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED = 7                                                                       # tests/test_wgrad_exact_host.py certifies the same cases
SMALL_P = (1, 2, 15, 16, 17, 31, 32, 33, 127, 128, 129, 1024, 1025, 2049)
WIDE_P = (1, 16, 32, 64, 128)
PLAN_P = (20011, 2 ** 18, 2 ** 18 + 1)
RANGE_P = (160, 4111)
MODE_KW = {"fp32": dict(wgrad_bf16=False), "bf16": dict(wgrad_bf16=True), "bf16x3": dict(wgrad_bf16="bf16x3"),
           "f16x2": dict(wgrad_bf16="f16x2", dgrad_h2=True)}
INF_WORD = 0x7f800000
_results = {}            # (P, family) -> {mode: ([24 cpu tensors], failure message or None)}: what the agreement test compares
_current = {}            # the one prepared small case (its buffers are reused by the four modes)


def _to(case, dev):
    return {k: ([t.to(dev) for t in v] if isinstance(v, list) else v.to(dev) if torch.is_tensor(v) else v) for k, v in case.items()}


def _want(case):
    """reference(case) rounded to fp32 -- after checking that the rounding changes nothing"""
    ref = C.reference(case)
    want = [r.float() for r in ref]
    for name, r, w in zip(C.TENSOR_NAMES, ref, want):
        assert torch.equal(w.double(), r), name + ": the expected value is no fp32 number"
    return want


def _pack(case, dwords="true", aword="true"):
    """Buffers of exactly the library's byte counts; every pointer the phase reads (x, the saved state, the scratch) is set."""
    from crnerf_amd import _lib
    lib = _lib.load()
    td, ta = C.true_words(case)
    return C.pack_state(case, lib.crnerf_mlp_train_acts_bytes(case["P"]), lib.crnerf_mlp_train_scratch_bytes(case["P"]),
                        td if isinstance(dwords, str) else dwords, ta if isinstance(aword, str) else aword)


def _wgrad(x, acts, scratch, mode):
    from crnerf_amd import ops
    with torch.no_grad():
        return ops.mlp_backward(None, x, None, None, acts, phase="wgrad", scratch=scratch, **MODE_KW[mode])


def _diff(case, bufs, mode, want):
    """phase="wgrad" on a packed case in one mode -> (the 24 tensors, one line per tensor that is not torch.equal to the reference: its name, the
    first differing index and both values)"""
    got = _wgrad(case["x"], bufs[0], bufs[1], mode)
    assert len(got) == 24
    return got, ["%s: %s" % (name, d) for name, g, w in zip(C.TENSOR_NAMES, got, want) for d in [C.first_difference(g, w)] if d is not None]


def _fail(what, mode, bad):
    return "%s, %s: %d of 24 tensors differ from float64\n  " % (what, mode, len(bad)) + "\n  ".join(bad)


def _run(case, bufs, mode, want, what):
    got, bad = _diff(case, bufs, mode, want)
    assert not bad, _fail(what, mode, bad)
    return got


def _small(P, family):
    if _current.get("key") != (P, family):
        case = _to(C.make_case(P, family, SEED), DEV)
        _current.clear()
        _current.update(key=(P, family), case=case, want=_want(case), bufs=_pack(case))
    return _current["case"], _current["bufs"], _current["want"]


def _small_mode(P, family, mode):
    """(the mode's 24 tensors on the CPU, its failure message or None), computed once"""
    res = _results.setdefault((P, family), {})
    if mode not in res:
        case, bufs, want = _small(P, family)
        got, bad = _diff(case, bufs, mode, want)
        res[mode] = ([g.cpu() for g in got], _fail("%s P=%d" % (family, P), mode, bad) if bad else None)
    return res[mode]


# ------------------------------------------------------------------------------------------------------------------ 1. layout guard
@pytest.mark.parametrize("core,mode", [("f32", "fp32"), ("h2", "f16x2")])
def test_helper_layout_is_the_products(core, mode):
    """A real state (mlp_forward_train + phase="dgrad"), unpacked and packed again into fresh buffers, gives the same weight gradients bit for bit;
    and the range words the h2 data gradient left are the bits of max |delta| per slot."""
    import crnerf_amd.synth as synth
    from crnerf_amd import ops
    from oracle import cpu_ref as O
    P = 300
    rng = np.random.default_rng(3)
    dev = {k: torch.from_numpy(np.ascontiguousarray(v)).to(DEV) for k, v in synth.mlp_state(13, 2.0, 0.5).items()}
    x = torch.cat([O.posenc(torch.from_numpy(rng.uniform(-2, 2, (P, 3)).astype(np.float32)), 15),
                   O.posenc(torch.from_numpy(rng.uniform(-1, 1, (P, 3)).astype(np.float32)), 4)], 1).to(DEV)
    d_out = torch.from_numpy(rng.normal(size=(P, 65)).astype(np.float32)).to(DEV)
    with torch.no_grad():
        out, acts = ops.mlp_forward_train(ops.pack_mlp_weights(dev), x)
        pk = ops.pack_mlp_weights_t_h2(dev) if core == "h2" else ops.pack_mlp_weights_t(dev)
        scratch = ops.mlp_backward(pk, None, out, d_out, acts, phase="dgrad", **MODE_KW[mode])
    first = _wgrad(x, acts, scratch, mode)
    st = C.unpack_state(x, acts, scratch, P)
    assert all(bool(torch.isfinite(a[:, :128]).all()) and bool(a.any()) for a in st["acts"]) and all(bool(d[:, :128].any()) for d in st["deltas"])
    acts2, scratch2 = C.pack_state(st, acts.numel(), scratch.numel(), st["dmax_words"], st["amax_word"])
    assert acts2.data_ptr() != acts.data_ptr() and scratch2.data_ptr() != scratch.data_ptr()
    again = _wgrad(st["x"], acts2, scratch2, mode)
    for name, a, b in zip(C.TENSOR_NAMES, first, again):
        assert bool(torch.isfinite(a).all()) and bool(a.any()), name
        assert torch.equal(a, b), "%s: %s" % (name, C.first_difference(b, a))
    if core == "h2":
        tensors = st["deltas"][:9] + [st["deltas"][9][:, :128], st["d_rgb"]]
        assert st["dmax_words"][:C.RANGE_USED] == [C.range_word(t) for t in tensors]
    # a mis-set helper would show: the same state with two delta slots swapped gives other gradients
    st["deltas"][1], st["deltas"][2] = st["deltas"][2], st["deltas"][1]
    acts3, scratch3 = C.pack_state(st, acts.numel(), scratch.numel(), st["dmax_words"], st["amax_word"])
    swapped = _wgrad(st["x"], acts3, scratch3, "fp32")
    assert not torch.equal(swapped[2], _wgrad(x, acts, scratch, "fp32")[2])


# ------------------------------------------------------------------------------------------------------------------ 2. small sizes
@pytest.mark.parametrize("mode", C.MODES)                       # (the top decorator varies fastest: a case is built once for its four modes)
@pytest.mark.parametrize("family", ["narrow", "narrow_signed"])
@pytest.mark.parametrize("P", SMALL_P)
def test_small_sizes_are_exact(mode, family, P):
    """One k-step, one prefetch group, one 32-point unit, a second chunk that holds a single point, 9 and 17 partials into the reduce (which keeps
    8 loads in flight).  f16x2: the range words are the true maxima."""
    err = _small_mode(P, family, mode)[1]
    assert err is None, err


# ------------------------------------------------------------------------------------------------------------------ 3. wide families
@pytest.mark.parametrize("P,family", [(P, f) for f in C.FAMILIES if f.startswith("wide") for P in WIDE_P if P <= C.FAMILIES[f]["max_P"]])
def test_wide_families_are_exact(P, family):
    """Second and third bf16 pieces, second fp16 pieces -- in the modes each family is fair for (single-piece bf16 is not among them)."""
    case = _to(C.make_case(P, family, SEED), DEV)
    C.certificate(case)
    modes = C.FAMILIES[family]["modes"]
    assert set(modes) <= set(C.fair_modes(case)) and "bf16" not in modes
    want, bufs = _want(case), _pack(case)
    for mode in modes:
        _run(case, bufs, mode, want, "%s P=%d" % (family, P))


# ------------------------------------------------------------------------------------------------------------------ 4. plans
def _plan_modes(P):
    """All four modes at one large size: data and float64 reference built once on the device; the buffers are freed afterwards."""
    key = (P, "narrow_signed")
    if key in _results and len(_results[key]) == 4:
        return _results[key]
    f = C.FAMILIES["narrow_signed"]
    assert C.closed_form_bits(P, f["md"], f["ma"]) < 24.0
    t0 = time.perf_counter()
    case = C.make_case(P, "narrow_signed", SEED, device=DEV)
    assert max(float(d.abs().max()) for d in case["deltas"] + [case["d_rgb"], case["d_sig"]]) == f["md"]          # what the closed form assumes
    assert max(float(a.abs().max()) for a in case["acts"] + [case["x"]]) == f["ma"]
    want = _want(case)                          # (integer data: rocBLAS's summation order is irrelevant; _want asserts reference == reference.float().double())
    bufs = _pack(case)
    x = case["x"]
    case = {"x": x, "P": P}
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    res = _results.setdefault(key, {})
    try:
        for mode in C.MODES:
            got, bad = _diff(case, bufs, mode, want)
            res[mode] = ([g.cpu() for g in got], _fail("narrow_signed P=%d" % P, mode, bad) if bad else None)
    finally:
        del bufs, want, x, case
        torch.cuda.empty_cache()
    print("\nP=%d: data + reference + packing %.2f s, four modes %.2f s" % (P, t1 - t0, time.perf_counter() - t1))
    return res


@pytest.mark.parametrize("P", PLAN_P)
def test_plans_are_exact(P):
    """20011: the batched plan with every job's chunk above 128, different between jobs, and a ragged last chunk.  2^18: the last batched size.
    2^18 + 1: the first size of the per-layer plan (CRNERF_WGRAD_BATCH is read once per process, so the size is the only way there); the narrow
    f16x2 jobs run on half chunks."""
    errs = [e for _, e in _plan_modes(P).values() if e is not None]
    assert not errs, "\n".join(errs)


# ------------------------------------------------------------------------------------------------------------------ 5. fabricated range words
_range_base = {}


def _range_case(P):
    if P not in _range_base:
        case = _to(C.make_case(P, "narrow", SEED), DEV)
        _range_base[P] = (case, _want(case), C.true_words(case))
    return _range_base[P]


@pytest.mark.parametrize("P", RANGE_P)
@pytest.mark.parametrize("variant", ["delta words zero", "activation word zero", "activation word Inf", "delta words two binades low"])
def test_f16x2_is_exact_whatever_the_words_say(variant, P):
    """Zero delta words: the kernel falls back by itself (and equals the bf16x3 run).  Activation word zero or Inf: scale 1.  Delta words that
    understate by two binades: the scaled deltas are still inside fp16, no fallback needed."""
    case, want, (td, ta) = _range_case(P)
    lower = lambda w, k: w - (k << 23)                                          # noqa: E731  (the word of a maximum 2^k times smaller)
    dwords, aword = {"delta words zero": ([0] * C.RANGE_USED, ta), "activation word zero": (td, 0), "activation word Inf": (td, INF_WORD),
                     "delta words two binades low": ([lower(w, 2) for w in td], ta)}[variant]
    bufs = _pack(case, dwords, aword)
    got = _run(case, bufs, "f16x2", want, "narrow P=%d, %s" % (P, variant))
    if variant == "delta words zero":
        x3 = _run(case, bufs, "bf16x3", want, "narrow P=%d, %s" % (P, variant))
        assert all(torch.equal(a, b) for a, b in zip(got, x3))


@pytest.mark.parametrize("P", RANGE_P)
@pytest.mark.parametrize("where", ["last point of the last whole 32-point unit", "first point"])
@pytest.mark.parametrize("operand", ["delta", "activation"])
def test_f16x2_throws_away_the_sums_of_a_wave_that_saw_fp16_overflow(operand, where, P):
    """One operand value four binades beyond what its range word promises -- 2^17 and more once scaled, past fp16's 65504 -- in a single point: "a
    wave that saw an operand leave fp16's range throws its sums away" and runs its chunk again on bf16x3; every other chunk keeps its f16x2 sums.
    The outlier sits in a full 256 x 256 job (delta slot 2 / activation slot 1: xyz_encoding_3) and in a narrow job (d_rgb / a direction column of x)."""
    base, _, (td, ta) = _range_case(P)
    p = (P // 32) * 32 - 1 if where.startswith("last") else 0
    case = dict(base, deltas=list(base["deltas"]), acts=list(base["acts"]))
    if operand == "delta":
        case["deltas"][2], case["d_rgb"] = base["deltas"][2].clone(), base["d_rgb"].clone()
        case["deltas"][2][p, 200] = 32.0
        case["d_rgb"][p, 63] = -32.0
    else:
        case["acts"][1], case["x"] = base["acts"][1].clone(), base["x"].clone()
        case["acts"][1][p, 129] = 240.0
        case["x"][p, 100] = 240.0
    C.certificate(case)
    assert set(C.MODES) <= set(C.fair_modes(case))                             # (with the TRUE words of the changed case)
    want = _want(case)
    bufs = _pack(case, td, ta)                                                 # the words of the case without the outlier: four binades low
    got = _run(case, bufs, "f16x2", want, "narrow P=%d, %s beyond its word at the %s" % (P, operand, where))
    x3 = _run(case, bufs, "bf16x3", want, "narrow P=%d, %s outlier" % (P, operand))
    assert all(torch.equal(a, b) for a, b in zip(got, x3))


# ------------------------------------------------------------------------------------------------------------------ 6. modes agree
@pytest.mark.parametrize("P,family", [(P, f) for P in SMALL_P for f in ("narrow", "narrow_signed")] + [(P, "narrow_signed") for P in PLAN_P])
def test_modes_agree(P, family):
    """Implied by the tests above; the message says which mode is the odd one out."""
    res = _plan_modes(P) if P in PLAN_P else {m: _small_mode(P, family, m) for m in C.MODES}
    res = {m: res[m][0] for m in C.MODES}
    lines = []
    for k, name in enumerate(C.TENSOR_NAMES):
        same = {m: [n for n in C.MODES if torch.equal(res[m][k], res[n][k])] for m in C.MODES}
        if any(len(v) != 4 for v in same.values()):
            odd = [m for m in C.MODES if len(same[m]) == 1]
            lines.append("%s: odd one(s) out %s; %s" % (name, odd or "(two camps)", "; ".join(
                "%s vs %s: %s" % (C.MODES[0], m, C.first_difference(res[m][k], res[C.MODES[0]][k])) for m in C.MODES[1:] if m not in same[C.MODES[0]])))
    assert not lines, "%s P=%d\n  " % (family, P) + "\n  ".join(lines)

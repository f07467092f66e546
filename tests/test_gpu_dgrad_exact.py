"""The MLP data gradients -- mlp_backward16_kernel (csrc/mlp_train16.hip), mlp_backward_h2_kernel, mlp_backward_x3_kernel -- held to the float64
chain BIT FOR BIT, per point: the ten delta rows (slot 9: its 128 columns), d_rgb and d_sig that ops.mlp_backward(phase="dgrad") leaves in the
scratch buffer, on inputs for which every fp32 summation order is exact (tests/_dgrad_cases.py: construction, certificate, reference, the relu-bit
map; tests/test_dgrad_exact_host.py: the same certificates on the CPU and the reference's tie to autograd).  out, d_out and the relu bits are
written by the test; nothing here comes from a forward except in the layout guard, which ties the test's bit writer to the product's.

torch.equal leaves no room for a relu bit read from the neighbouring lane group or the wrong tile, a mask on the linear slot, a sigma-head term
missed in one tile, a delta piece stored into another row, a tile of the persistent loop done twice or not at all (the sizes reach iters = 3), or
an h2 range word that is not the true maximum: each changes single points or single 4-column groups, which the weight-gradient sums of the
autograd-oracle tests dilute by 1 / n.

Every case is certified on the device before it is used (sum |terms| < 2^24 quanta per point and sum), and a core runs a case only when
fair_cores() finds its piece products complete on that case's data; fp32 runs everything.

The forward twin (last section): ops.mlp_forward_train's ten saved rows and relu words on integer inputs, bit for bit, and `out` to four times the
fp32 CPU oracle's own error.

MEASURED on an MI355X (256 compute units) when these tests were written: the fp32, h2 and x3 kernels return the float64 bits on every case they are
fair for -- h2 sits out six of the sixteen wide18 sizes (1, 16, 127, 128, 129 and 128 C points), where some row of 22 significant bits does not
split into two fp16 pieces under its point's scale, and runs everything else; x3 and fp32 run everything --, the range words are the true maxima, the forward twin's rows and relu words are exact and its `out` is 8e-8 from float64
(bar 3.2e-7).  The whole file takes 7 s, the largest cases 0.05 s a test.  Mutation check (scratch builds, one value-only line each; "oracle" =
test_mlp_backward_vs_autograd_oracle and test_split_core_backward_vs_autograd_oracle of test_gpu_parity.py, "cross" = the h2 / x3 "matches the fp32
data gradient" tests, which reach 70,000 points):
  the f16x2 range word floored to a power of two in point_scale_h        red here (12 tests), oracle, cross and the f16x2 oracle tests green
  sigma-head fmaf without d_sig in tile 5 from the loop's second round:
      fp32 kernel                                                        red here (12), oracle green, cross red at 70,000 only
      h2 kernel                                                          red here (15), oracle green, cross red at 70,000 only
  x3 kernel: sigma head without d_sig for one point in 256               red here (26), oracle red for x3, cross red from 4,099 points on
  fp32 kernel: mask bit 4 T + (r ^ 1)                                    red here (66) and in the older tests
  h2 kernel: inv applied twice in finish_delta_h                         red here (72) and in the older tests
  x3 kernel: sigma head skipped for tile 3                               red here (69) and in the older tests
"""
import pytest
import torch

import _dgrad_cases as C
import _wgrad_cases as WG

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED = 7                                                                       # tests/test_dgrad_exact_host.py certifies the same cases
SMALL_P = (1, 15, 16, 17, 31, 32, 33, 127, 128, 129, 257)
LARGE_P = ("128C-1", "128C", "128C+1", "128C+129", "256C+1")                   # C: the device's compute units; 256C+1: three rounds of the persistent loop
CORE_KW = {"fp32": {}, "h2": dict(dgrad_h2=True), "x3": dict(dgrad_x3=True)}
_current = {}            # the one prepared case (its buffers are reused by the three cores)
_packs = {}              # (family, core) -> transposed pack


def _points(P):
    if not isinstance(P, str):
        return P
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    return {"128C-1": 128 * cus - 1, "128C": 128 * cus, "128C+1": 128 * cus + 1, "128C+129": 128 * cus + 129, "256C+1": 256 * cus + 1}[P]


def _pack_t(weights, core):
    from crnerf_amd import ops
    st = dict(zip(C.TENSOR_NAMES, weights))
    with torch.no_grad():
        return {"fp32": ops.pack_mlp_weights_t, "h2": ops.pack_mlp_weights_t_h2, "x3": ops.pack_mlp_weights_t_x3}[core](st)


def _state(case, fill=0xff):
    """(saved state, scratch) of exactly the library's byte counts: the case's relu bits in place, every other byte 0xff -- activation rows a data
    gradient has no business reading, and deltas / range words that read as NaN / garbage until a kernel writes them."""
    from crnerf_amd import _lib
    lib = _lib.load()
    P = case["P"]
    acts = torch.full((lib.crnerf_mlp_train_acts_bytes(P),), fill, dtype=torch.uint8, device=DEV)
    C.pack_bits(acts, case["bits"], P)
    return acts, torch.full((lib.crnerf_mlp_train_scratch_bytes(P),), fill, dtype=torch.uint8, device=DEV)


def _prepare(P, family):
    key = (P, family)
    if _current.get("key") != key:
        _current.clear()
        torch.cuda.empty_cache()
        case = C.make_case(_points(P), family, SEED, device=DEV)
        bits = C.certificate(case)
        ref = C.reference(case)
        want, fair, words = C.expected32(ref), C.fair_cores(case, ref), C.range_words(ref)
        del ref
        acts, scratch = _state(case)
        _current.update(key=key, case=case, want=want, fair=fair, words=words, acts=acts, scratch=scratch, bits=max(bits.values()))
    return _current


def _views(scratch, P):
    L = C.layout(P)
    f = lambda b0, n: scratch[b0:b0 + 4 * n].view(torch.float32)               # noqa: E731
    return {"deltas": f(0, C.SLOTS * P * C.W).view(C.SLOTS, P, C.W), "d_rgb": f(L["d_rgb"], P * C.FEAT).view(P, C.FEAT), "d_sig": f(L["d_sig"], P),
            "words": [int(w) & 0xffffffff for w in scratch[L["dmax"]:L["dmax"] + 4 * WG.RANGE_USED].view(torch.int32).cpu()]}


def _differences(scratch, P, want):
    """One line per output that is not torch.equal to the reference: its name, how many elements differ, the first (point, column), both values."""
    got = _views(scratch, P)
    pairs = [("slot %d" % s, got["deltas"][s][:, :want["deltas"][s].shape[1]], want["deltas"][s]) for s in range(C.SLOTS)]
    pairs += [("d_rgb", got["d_rgb"], want["d_rgb"]), ("d_sig", got["d_sig"], want["d_sig"])]
    return ["%s: %s" % (name, d) for name, g, w in pairs for d in [C.first_difference(g, w)] if d is not None]


def _dgrad(case, core, acts, scratch, pack=None, **kw):
    from crnerf_amd import ops
    if pack is None:
        pack = _packs.get((case["family"], core))
        if pack is None:
            pack = _packs[(case["family"], core)] = _pack_t(case["weights"], core)
    with torch.no_grad():
        res = ops.mlp_backward(pack, None, case["out"], case["d_out"], acts, phase="dgrad", scratch=scratch, **dict(CORE_KW[core], **kw))
    assert res.data_ptr() == scratch.data_ptr()
    return res


# ------------------------------------------------------------------------------------------------------------------ 1. layout guard
def test_the_bit_writer_is_the_products():
    """On a real ops.mlp_forward_train state the saved words of slots 0-7 and 9 are `acts > 0` under the helper's bit map (slot 9: bits 32..63
    clear), and the helper's reader undoes its writer.  Without this a wrong map in the helper would make the tests below test the helper."""
    import numpy as np
    import crnerf_amd.synth as synth
    from crnerf_amd import ops
    from oracle import cpu_ref as O
    P = 333
    rng = np.random.default_rng(3)
    dev = {k: torch.from_numpy(np.ascontiguousarray(v)).to(DEV) for k, v in synth.mlp_state(13, 2.0, 0.5).items()}
    x = torch.cat([O.posenc(torch.from_numpy(rng.uniform(-2, 2, (P, 3)).astype(np.float32)), 15),
                   O.posenc(torch.from_numpy(rng.uniform(-1, 1, (P, 3)).astype(np.float32)), 4)], 1).to(DEV)
    with torch.no_grad():
        out, acts = ops.mlp_forward_train(ops.pack_mlp_weights(dev), x)
    st = C.unpack_state(x, acts, torch.zeros(C.layout(P)["ws"], dtype=torch.uint8, device=DEV), P)
    words = C.unpack_bits(acts, P)
    for s in range(C.SLOTS):
        if s == 8:
            continue
        on = st["acts"][s][:, :128 if s == 9 else C.W] > 0
        assert 0.05 < float(on.float().mean()) < 0.95, s                         # a state with both kinds of bits
        assert torch.equal(words[s], C.mask_to_bits(on)), "slot %d: %s" % (s, C.first_difference(words[s], C.mask_to_bits(on)))
        assert torch.equal(C.bits_to_mask(words[s])[:, :on.shape[1]], on)
    again = torch.zeros_like(acts)
    C.pack_bits(again, words, P)
    L = C.layout(P)
    assert torch.equal(again[L["masks"]:L["amax"]], acts[L["masks"]:L["amax"]]) and not bool(again[:L["masks"]].any())


# ------------------------------------------------------------------------------------------------------------------ 2. bit equality per core
@pytest.mark.parametrize("core", C.CORES)                       # (the top decorator varies fastest: a case is built once for its three cores)
@pytest.mark.parametrize("family", list(C.FAMILIES))
@pytest.mark.parametrize("P", SMALL_P + LARGE_P)
def test_deltas_are_exact(core, family, P):
    """1: a single lane.  15..33: the fp32 kernel's 16-point tiles and the split cores' 32-point tiles, one short, full, one over.  127..129, 257:
    a workgroup's 128 points.  128 C +- 1: the last single-round grid and the first launch whose loop runs twice (one workgroup, then two, do a
    second tile against the weight ring wrapped from the first).  256 C + 1: three rounds."""
    cur = _prepare(P, family)
    case = cur["case"]
    if core not in cur["fair"]:
        assert (family, core) == ("wide18", "h2"), "only wide18's 22-bit rows may be too wide, and only for two fp16 pieces"
        print("\n%s P=%d: not fair for %s, left out" % (family, case["P"], core))
        return                                                  # this core's pieces cannot hold this case's data (decided by fair_cores on the data)
    cur["scratch"].fill_(0xff)
    _dgrad(case, core, cur["acts"], cur["scratch"])
    bad = _differences(cur["scratch"], case["P"], cur["want"])
    assert not bad, "%s P=%d (%.1f bits), %s: %d of 12 outputs differ from float64\n  " % (family, case["P"], cur["bits"], core, len(bad)) + "\n  ".join(bad)


# ------------------------------------------------------------------------------------------------------------------ 3. range words
@pytest.mark.parametrize("family", ["narrow", "wide3", "wide12"])
@pytest.mark.parametrize("P", (1, 33, 257, "128C+1"))
def test_h2_leaves_the_true_maxima_in_the_range_words(family, P):
    """With the f16x2 flag the h2 data gradient leaves, per delta slot and for d_rgb, the bits of the largest |value| it wrote: equal to the
    exact deltas' maxima.  The words held 0xffffffff before the call."""
    cur = _prepare(P, family)
    case = cur["case"]
    assert "h2" in cur["fair"]
    cur["scratch"].fill_(0xff)
    assert _views(cur["scratch"], case["P"])["words"] == [0xffffffff] * WG.RANGE_USED
    _dgrad(case, "h2", cur["acts"], cur["scratch"], wgrad_bf16="f16x2")
    bad = _differences(cur["scratch"], case["P"], cur["want"])
    assert not bad, "\n".join(bad)
    got = _views(cur["scratch"], case["P"])["words"]
    assert got == cur["words"], "range words (slots 0..9, d_rgb): got %s, want %s" % (["%08x" % w for w in got], ["%08x" % w for w in cur["words"]])


# ------------------------------------------------------------------------------------------------------------------ 4. refused h2 pack
@pytest.mark.parametrize("P", (33, 257, "128C+1"))
def test_a_refused_h2_pack_hands_over_to_the_x3_stand_in(P):
    """One weight of xyz_encoding_4 at 256: the h2 pack carries its range flag, the h2 kernel returns at once and the x3 kernel behind it
    (fallback_t_x3, gated on the device by the flag word) writes the deltas -- bit-equal to float64 again."""
    from crnerf_amd import ops
    case = C.make_case(_points(P), "wide3", SEED, device=DEV)
    w4 = case["weights"][C.TENSOR_NAMES.index("xyz_encoding_4.0.weight")]
    r, c = (int(v) for v in (w4 != 0).nonzero()[5])
    w4[r, c] = 256.0 * float(w4[r, c].sign())
    C.certificate(case)
    ref = C.reference(case)
    fair = C.fair_cores(case, ref)
    assert "x3" in fair and "h2" not in fair
    want = C.expected32(ref)
    del ref
    acts, scratch = _state(case)
    pk = _pack_t(case["weights"], "h2")
    assert not ops.pack_h2_in_range(pk)
    _dgrad(case, "h2", acts, scratch, pack=pk, fallback_t_x3=_pack_t(case["weights"], "x3"))
    bad = _differences(scratch, case["P"], want)
    assert not bad, "wide3 with a weight of 256, P=%d: %d of 12 outputs differ\n  " % (case["P"], len(bad)) + "\n  ".join(bad)
    assert bool(want["deltas"][2][:, c].any())                   # the large weight is on the chain


# ------------------------------------------------------------------------------------------------------------------ 5. whole backward vs. two phases
@pytest.mark.parametrize("core", C.CORES)
@pytest.mark.parametrize("P", (33, 129))
def test_whole_backward_equals_dgrad_then_wgrad(core, P):
    """A written case with integer x and activation rows (tests/_wgrad_cases.py) beside the relu bits: phase="dgrad" then phase="wgrad" give the 24
    gradients of the one-call backward, and both are the float64 sums over the float64 deltas."""
    from crnerf_amd import _lib, ops
    lib = _lib.load()
    case = C.make_case(P, "wide3", SEED, device=DEV)
    assert core in C.fair_cores(case)
    ref = C.reference(case)
    wcase = WG.make_case(P, "narrow", SEED, device=DEV)
    wcase["deltas"] = [torch.nn.functional.pad(d, (0, C.W - d.shape[1])).float() for d in ref["deltas"]]
    wcase["d_rgb"], wcase["d_sig"] = ref["d_rgb"].float(), ref["d_sig"].float()
    bits = C.wgrad_certificate(wcase)
    want = [r.float() for r in WG.reference(wcase)]
    acts, _ = WG.pack_state(wcase, lib.crnerf_mlp_train_acts_bytes(P), lib.crnerf_mlp_train_scratch_bytes(P))
    C.pack_bits(acts, case["bits"], P)
    _, scratch = _state(case)
    pk = _pack_t(case["weights"], core)
    with torch.no_grad():
        _dgrad(case, core, acts, scratch, pack=pk)
        two = ops.mlp_backward(None, wcase["x"], None, None, acts, phase="wgrad", scratch=scratch, **CORE_KW[core])
        whole = ops.mlp_backward(pk, wcase["x"], case["out"], case["d_out"], acts, **CORE_KW[core])
    for name, a, b, w in zip(C.TENSOR_NAMES, two, whole, want):
        assert torch.equal(a, b), "%s, two phases vs. one call: %s" % (name, C.first_difference(a, b))
        assert torch.equal(a, w), "%s vs. float64 (%.1f bits): %s" % (name, max(bits.values()), C.first_difference(a, w))


# ------------------------------------------------------------------------------------------------------------------ 6. the forward twin
_bar = []


def _out_bar():
    if not _bar:
        from oracle import cpu_ref as O
        _bar.append(C.out_bar(O.mlp_forward, SEED))
    return _bar[0]


@pytest.mark.parametrize("P,shift", [(P, 0.0) for P in SMALL_P + ("128C+1",)] + [(P, C.SIGMA_HIGH) for P in (1, 33, 257, "128C+1")])
def test_forward_twin_rows_and_relu_bits_are_exact(P, shift):
    """ops.mlp_forward_train on integer x, weights +-1 and integer biases: the ten saved rows (slot 9: 128 columns) and the relu words of slots 0-7
    and 9 equal float64 bit for bit -- about a third of the pre-activations are exactly 0, where the rule is `> 0` --, and `out` is within four
    times the fp32 CPU oracle's own error of float64 sigmoid / softplus of the exact pre-activations (shift: the sigma pre-activations lie around
    softplus's threshold of 20, beyond which softplus(x) = x; a path of the epilogue, not of the tiling: four sizes)."""
    from crnerf_amd import ops
    case = C.make_forward_case(_points(P), SEED, device=DEV, sigma_shift=shift)
    n = case["P"]
    ref = C.forward_reference(case)
    C.forward_certificate(case, ref)
    assert not shift or n < 33 or float(ref["pre_sig"].max()) > 20.0
    with torch.no_grad():
        out, acts = ops.mlp_forward_train(ops.pack_mlp_weights(C.state_dict(case)), case["x"])
    L = C.layout(n)
    rows = acts[:L["masks"]].view(torch.float32).view(C.SLOTS, n, C.W)
    words = C.unpack_bits(acts, n)
    bad = []
    for s in range(C.SLOTS):
        want = ref["acts"][s].float()
        d = C.first_difference(rows[s][:, :want.shape[1]], want)
        if d is not None:
            bad.append("row %d: %s" % (s, d))
        if s != 8:
            d = C.first_difference(words[s], ref["bits"][s])
            if d is not None:
                bad.append("relu words %d (point, word): %s" % (s, d))
    assert not bad, "forward P=%d: " % n + "\n  ".join(bad)
    bar, oracle_err = _out_bar()
    err = float((out.double() - ref["out"]).abs().max())
    print("\nforward P=%d shift %g: out error %.3g, bar %.3g (oracle %.3g)" % (n, shift, err, bar, oracle_err))
    assert err <= bar, (err, bar)

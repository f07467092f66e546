"""CPU half of the bit-exact data-gradient tests (tests/_dgrad_cases.py holds the construction and its reasoning): every family is certified at
every point count that tests/test_gpu_dgrad_exact.py uses (the sums are per point, so the closed form from the weights alone covers the sizes that
depend on the device), the float64 chain is float64 autograd's backward of oracle.cpu_ref.mlp_forward, an fp32 evaluation in two summation orders
already equals it bit for bit, the cases are what the module says they are, and a numpy emulation of the kernels' index arithmetic reproduces the
reference while seven one-line slips of it do not."""
import numpy as np
import pytest
import torch

import _dgrad_cases as C

SMALL_P = (1, 15, 16, 17, 31, 32, 33, 127, 128, 129, 257)                      # test_gpu_dgrad_exact.py: SMALL_P
LARGE_P = (128 * 256 + 129, 256 * 256 + 1)                                     # two of the sizes that follow the device's 256 compute units
SEED = 7


# ------------------------------------------------------------------------------------------------------------------ certificates
@pytest.mark.parametrize("family", list(C.FAMILIES))
def test_every_gpu_case_is_certified(family):
    closed = C.closed_form_bits(C.make_weights(family, SEED), C.FAMILIES[family]["gm"] + 3)
    assert max(closed.values()) < 24.0
    lines = []
    for P in SMALL_P + (2049,):
        case = C.make_case(P, family, SEED)
        bits = C.certificate(case)
        assert float(case["d_out"].abs().max()) == C.FAMILIES[family]["gm"] + 3          # what the closed form assumes
        assert all(bits[s] <= closed[s] + 1e-9 for s in range(C.SLOTS)), (P, bits, closed)
        lines.append("P=%d: worst %.2f bits (slot %d)" % (P, max(bits.values()), max(bits, key=bits.get)))
    print("\n%s: closed form %.2f bits for any P, margin %.2f\n  " % (family, max(closed.values()), 24 - max(closed.values())) + "\n  ".join(lines))


@pytest.mark.parametrize("P", LARGE_P)
def test_a_large_case_is_certified_in_full_too(P):
    """The device-dependent sizes are certified on the device before use; here one family is built at such sizes on the CPU as well."""
    case = C.make_case(P, "wide18", SEED)
    bits = C.certificate(case)
    closed = C.closed_form_bits(case["weights"], C.FAMILIES["wide18"]["gm"] + 3)
    assert max(bits.values()) <= max(closed.values()) < 24.0


def test_a_case_beyond_the_bound_fails_the_certificate():
    case = C.make_case(33, "wide18", SEED)
    C.certificate(case)
    case["d_out"][5, :64] = 2.0 ** 22 + 1.0                                     # 23-bit gradients: four more bits than the family's
    case["out"][5, :64] = 0.25
    with pytest.raises(AssertionError, match="needs|no fp32 number"):
        C.certificate(case)
    case = C.make_case(33, "narrow", SEED)
    case["out"][3, 64] = 1.0                                                    # a softplus' that is neither 0 nor 1
    with pytest.raises(AssertionError):
        C.certificate(case)


# ------------------------------------------------------------------------------------------------------------------ the chain is autograd's backward
class _Recorder:
    """torch.nn.functional as oracle.cpu_ref sees it, with every F.linear output kept for its gradient"""

    def __init__(self):
        self.kept = []

    def linear(self, x, w, b):
        y = torch.nn.functional.linear(x, w, b)
        y.retain_grad()
        self.kept.append(y)
        return y

    def __getattr__(self, name):
        return getattr(torch.nn.functional, name)


def test_the_chain_is_float64_autograd_of_the_oracle(monkeypatch):
    """A random dense net, a real float64 forward through oracle.cpu_ref.mlp_forward: reference() fed with that forward's out and its h > 0 bits
    equals autograd's gradients at the hidden activations (masked by h > 0 where the layer has a relu) to 1e-12 of each tensor's largest entry."""
    from oracle import cpu_ref as O
    P = 97
    gen = torch.Generator().manual_seed(11)
    w = {}
    for name, shape in zip(C.TENSOR_NAMES, C.SHAPES):
        fan_in = shape[1] if len(shape) == 2 else 1
        w[name] = (torch.randn(shape, generator=gen, dtype=torch.float64) * ((2.0 / fan_in) ** 0.5 if len(shape) == 2 else 0.1)).requires_grad_(True)
    x = torch.randn(P, 120, generator=gen, dtype=torch.float64)
    d_out = torch.randn(P, 65, generator=gen, dtype=torch.float64)
    rec = _Recorder()
    monkeypatch.setattr(O, "F", rec)
    out = O.mlp_forward(w, x)
    (out * d_out).sum().backward()
    # F.linear calls in order: xyz_encoding_1..8, static_sigma, xyz_encoding_final, dir_encoding, static_rgb
    assert len(rec.kept) == 12
    hidden = rec.kept[:8] + [rec.kept[9], rec.kept[10]]                         # slots 0..9 (relu_ ran in place: the kept tensors are post-relu)
    sigma_pre = rec.kept[8]
    assert float(sigma_pre.detach().max()) < 20.0 and float(out.detach()[:, 64].min()) > 1e-3      # inside softplus's smooth branch, where 1 - exp(-sigma) is well conditioned
    bits = torch.zeros(C.SLOTS, P, 4, dtype=torch.int64)
    for s, h in enumerate(hidden):
        if s != 8:
            bits[s] = C.mask_to_bits(h.detach() > 0)
            assert 0.1 < float((h > 0).double().mean()) < 0.9
    case = {"P": P, "family": "dense", "weights": [w[n].detach() for n in C.TENSOR_NAMES], "out": out.detach(), "d_out": d_out, "bits": bits}
    ref = C.reference(case)
    close = lambda a, b: float((a - b).abs().max()) <= 1e-12 * float(b.abs().max())   # noqa: E731
    for s, h in enumerate(hidden):
        want = h.grad if s == 8 else h.grad * (h.detach() > 0)
        assert float(want.abs().max()) > 0 and close(ref["deltas"][s], want), s
    assert close(ref["d_rgb"], rec.kept[11].grad) and close(ref["d_sig"], sigma_pre.grad[:, 0])


# ------------------------------------------------------------------------------------------------------------------ summation order
@pytest.mark.parametrize("family", list(C.FAMILIES))
def test_fp32_in_two_summation_orders_gives_the_reference_to_the_bit(family):
    case = C.make_case(129, family, SEED)
    ref = C.reference(case)
    for order in ("plain", "reversed-chunked"):
        got = C.chain_fp32(case, order)
        assert all(d.dtype == np.float32 for d in got["deltas"]) and C.same(got, ref), order


# ------------------------------------------------------------------------------------------------------------------ the cases are what they say
@pytest.mark.parametrize("family", list(C.FAMILIES))
def test_the_weights_are_sparse_signed_and_distinct(family):
    f = C.FAMILIES[family]
    for name, w in zip(C.LAYERS, C.make_weights(family, SEED)[0::2]):
        nz = w != 0
        k = f["k_of"].get(name, f["k"])
        assert bool((w.abs() < 255).all()) and bool((w < 0).any()) and bool((w > 0).any()), name
        assert C.quantum(w) >= 1.0 / 16.0, name                                                     # integer or dyadic
        if name == "static_sigma.0":
            assert bool(nz.all()) and bool((w[0, 1:] != w[0, :-1]).all())
            continue
        assert bool((nz.sum(0) == k).all()), name                                                   # every column non-zero, k entries
        assert int(nz.sum(1).max()) <= -(-w.shape[1] // w.shape[0]) * k, name                        # bounded per row too
        assert not bool((nz[:, 1:] == nz[:, :-1]).all(0).any()), name                                # neighbouring columns: different supports
    w5, wd = (C.make_weights(family, SEED)[C.TENSOR_NAMES.index(n)] for n in ("xyz_encoding_5.0.weight", "dir_encoding.0.weight"))
    assert bool(w5[:, :C.XYZ].any(0).all()) and bool(wd[:, C.W:].any(0).all())                       # the columns the chain must NOT read are filled


@pytest.mark.parametrize("family", list(C.FAMILIES))
def test_the_points_are_what_the_docstring_says(family):
    gm, P = C.FAMILIES[family]["gm"], 300
    case = C.make_case(P, family, SEED)
    out, d, bits = case["out"], case["d_out"], case["bits"]
    assert set(out[:, :64].unique().tolist()) == {0.0, 0.25, 0.5, 0.75, 1.0} and set(out[:, 64].unique().tolist()) == {0.0, C.SIGMA_ON}
    assert bool((d == d.round()).all()) and 0.4 < float((d == 0).float().mean()) < 0.7
    zero_rows = (d == 0).all(1)
    assert 10 < int(zero_rows.sum()) < 80
    marked = torch.zeros(P, dtype=torch.bool)
    marked[15::16] = True
    marked[0] = marked[P - 1] = True
    assert bool((d[marked] != 0).all()) and bool((d[~marked].abs() <= gm).all())
    assert bool((d[15::16].abs() == gm + 1).all()) and bool((d[0].abs() == gm + 3).all()) and bool((d[P - 1].abs() == gm + 2).all())
    rows = {tuple(d[p].tolist()) for p in (0, P - 1, 15, 31, 127)}                                   # each kind of mark is a row of its own
    assert len(rows) == 5
    ref = C.reference(case)
    assert bool((ref["d_rgb"][marked] != 0).all()) and bool((ref["d_sig"][marked] != 0).all())
    assert bool((ref["d_sig"][(out[:, 64] == 0)] == 0).all()) and bool((ref["d_sig"] == d[:, 64].double() * (out[:, 64] > 0)).all())
    # the relu words: slot 8 clear, slot 9's upper halves the complement of the lower, everything else differs from its neighbours
    assert not bool(bits[8].any()) and bool((((bits[9] >> 32) & 0xffffffff) == (~bits[9] & 0xffffffff)).all())
    for s in range(C.SLOTS):
        if s == 8:
            continue
        assert bool((bits[s][1:] != bits[s][:-1]).all()) and bool((bits[s][:, 1:] != bits[s][:, :-1]).all()), s       # points, words
        assert s in (0, 9) or bool((bits[s] != bits[s - 1]).all()), s                                                # slots
        assert 0.45 < float(C.bits_to_mask(bits[s]).float().mean()) < 0.55
    assert all(bool(dl.any()) for dl in ref["deltas"])


def test_the_bit_map_and_its_inverse():
    """bit 4 T + r of word g <-> feature 16 T + 4 g + r (csrc/mlp_train16.h), spelled out"""
    words = torch.zeros(1, 4, dtype=torch.int64)
    words[0, 2] = 1 << 37                                                        # T = 9, r = 1, g = 2
    mask = C.bits_to_mask(words)
    assert mask.sum() == 1 and bool(mask[0, 16 * 9 + 4 * 2 + 1])
    full = torch.rand(5, 256, generator=torch.Generator().manual_seed(1)) < 0.5
    assert torch.equal(C.bits_to_mask(C.mask_to_bits(full)), full)
    half = C.mask_to_bits(full[:, :128])
    assert bool(((half >> 32) == 0).all()) and torch.equal(C.bits_to_mask(half)[:, :128], full[:, :128])
    P = 7
    buf = torch.zeros(C.layout(P)["acts_min"], dtype=torch.uint8)
    bits = C.make_case(P, "narrow", SEED)["bits"]
    C.pack_bits(buf, bits, P)
    assert torch.equal(C.unpack_bits(buf, P), bits)
    s, p, g = 6, 4, 3                                                            # masks[slot][point][g] behind the ten activation rows
    at = 10 * P * 1024 + ((s * P + p) * 4 + g) * 8
    assert int(buf[at:at + 8].view(torch.int64)[0]) == int(bits[s, p, g])


# ------------------------------------------------------------------------------------------------------------------ fairness
def test_fair_cores_follows_the_data():
    """narrow: single pieces everywhere, all three cores.  wide12: second pieces, still all three.  wide18: third bf16 pieces; two fp16 pieces
    under one per-point scale stop holding the rows once there are enough points for a 22-bit span to occur."""
    for family, P, want, pieces in (("narrow", 257, C.CORES, (1, 1)), ("wide3", 257, C.CORES, (2, 1)), ("wide12", 257, C.CORES, (2, 2)),
                                    ("wide18", 1, C.CORES, (2, 2)), ("wide18", 2049, ("fp32", "x3"), (3, 2))):
        case = C.make_case(P, family, SEED)
        ref = C.reference(case)
        assert C.fair_cores(case, ref) == want and C.pieces_used(ref) == pieces, (family, P, C.fair_cores(case, ref), C.pieces_used(ref))
    case = C.make_case(33, "wide3", SEED)
    w4 = case["weights"][C.TENSOR_NAMES.index("xyz_encoding_4.0.weight")]
    r, c = (int(v) for v in (w4 != 0).nonzero()[5])
    w4[r, c] = 256.0 * float(w4[r, c].sign())                                    # what the refused-pack test does
    C.certificate(case)
    assert C.fair_cores(case) == ("fp32", "x3")
    case = C.make_case(33, "wide18", SEED)
    case["weights"][C.TENSOR_NAMES.index("xyz_encoding_3.0.weight")] *= 1.0 + 2.0 ** -9      # two-piece weights against three-piece deltas
    assert C.fair_cores(case) == ("fp32",)


def test_point_scale_is_the_kernels():
    """2^(134 - e), e clamped to [32, 254]: the row's largest entry lands in [2^7, 2^8); a zero row keeps 2^102"""
    d = torch.tensor([[0.0, 0.0], [3.0, -0.5], [2.0 ** -100, 0.0], [255.0, 1.0]], dtype=torch.float64)
    sc = C.point_scale(d)[:, 0]
    assert sc.tolist() == [2.0 ** 102, 2.0 ** 6, 2.0 ** 102, 1.0]
    assert 128 <= 3.0 * 2.0 ** 6 < 256


# ------------------------------------------------------------------------------------------------------------------ teeth
@pytest.mark.parametrize("lanes", ["g4", "h2"])
@pytest.mark.parametrize("family", ["narrow", "wide3"])
def test_the_emulated_index_arithmetic_reproduces_the_reference_and_its_slips_do_not(family, lanes):
    for P in (1, 33):
        case = C.make_case(P, family, SEED)
        ref = C.reference(case)
        assert C.same(C.emulate(case, lanes), ref)
        for mutant in C.MUTANTS:
            assert not C.same(C.emulate(case, lanes, mutant), ref), (P, mutant)
    assert len(C.MUTANTS) >= 5


# ------------------------------------------------------------------------------------------------------------------ the forward twin
@pytest.mark.parametrize("shift", [0.0, C.SIGMA_HIGH])
def test_forward_cases_are_certified_and_tie_at_zero(shift):
    from oracle import cpu_ref as O
    for P in SMALL_P + (2049,):
        case = C.make_forward_case(P, SEED, sigma_shift=shift)
        ref = C.forward_reference(case)
        bits = C.forward_certificate(case, ref)
        assert bool((case["x"] == case["x"].round()).all()) and float(case["x"].abs().max()) <= 2
        got = O.mlp_forward({n: t.double() for n, t in zip(C.TENSOR_NAMES, case["weights"])}, case["x"].double())
        assert float((got - ref["out"]).abs().max()) <= 1e-15, P                 # the reference IS the oracle's forward, in float64
    print("\nforward, shift %g: worst %.2f bits (%s)" % (shift, max(bits.values()), max(bits, key=bits.get)))
    pres = []
    C.forward(case["weights"], case["x"], pres=pres)
    for s, pre in zip(list(range(8)) + [9], pres):
        tie, neg, pos = (float(m.double().mean()) for m in (pre == 0, pre < 0, pre > 0))
        assert tie > 0.08 and neg > 0.1 and pos > 0.2, (s, tie, neg, pos)         # the rule `> 0` is asked at 0 all the time
        assert float((ref["acts"][s].std(0) > 0).double().mean()) > 0.15, s      # and the rows depend on the point
    if shift:
        assert float(ref["pre_sig"].max()) > 20.0 >= float(ref["pre_sig"].min())           # both sides of the threshold
    else:
        assert set(ref["pre_rgb"].unique().tolist()) >= set(float(v) for v in range(-4, 5))


def test_the_out_bar_and_what_one_quantum_moves():
    """bar = min(1e-6, 4 x the fp32 CPU oracle's largest error on these cases); one quantum (1) of any head pre-activation inside the bound moves
    sigmoid / softplus by at least 1000 bars, and beyond the threshold softplus moves by the quantum itself."""
    from oracle import cpu_ref as O
    bar, err = C.out_bar(O.mlp_forward, SEED)
    print("\nfp32 CPU oracle against float64 on the forward cases: %.3g; bar %.3g" % (err, bar))
    assert 1e-9 < err < 2.5e-7 and bar <= 1e-6
    pre = torch.arange(-C.PRE_BOUND - 1, C.PRE_BOUND + 2, dtype=torch.float64)
    for f in (torch.sigmoid, torch.nn.functional.softplus):
        assert float((f(pre)[1:] - f(pre)[:-1]).abs().min()) >= 1000 * bar, f
    hi = torch.arange(C.SIGMA_HIGH - C.PRE_BOUND - 1, C.SIGMA_HIGH + C.PRE_BOUND + 2, dtype=torch.float64)
    sp = torch.nn.functional.softplus(hi)
    assert float((sp[1:] - sp[:-1]).min()) >= 0.99

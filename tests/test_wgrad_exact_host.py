"""CPU half of the bit-exact weight-gradient tests (tests/_wgrad_cases.py holds the construction and its reasoning): every case that
tests/test_gpu_wgrad_exact.py runs is certified -- in full up to P = 2049, by the closed-form bound for the three large sizes --, an fp32 numpy
evaluation in shuffled point orders and two chunkings already equals the float64 reference bit for bit on them, a case that breaks the bound
fails the certificate, the byte layout round-trips, and every family's mode list obeys the piece rules of the split modes."""
import numpy as np
import pytest
import torch

import _wgrad_cases as C

SMALL_P = (1, 2, 15, 16, 17, 31, 32, 33, 127, 128, 129, 1024, 1025, 2049)      # test_gpu_wgrad_exact.py: SMALL_P, WIDE_P, PLAN_P, RANGE_P
WIDE_P = (1, 16, 32, 64, 128)
PLAN_P = (20011, 2 ** 18, 2 ** 18 + 1)
RANGE_P = (160, 4111)
SEED = 7


def _gpu_cases():
    out = [(P, f) for P in SMALL_P + RANGE_P for f in ("narrow", "narrow_signed") if not (P in RANGE_P and f != "narrow")]
    return out + [(P, f) for f in C.FAMILIES if f.startswith("wide") for P in WIDE_P if P <= C.FAMILIES[f]["max_P"]]


@pytest.mark.parametrize("P,family", _gpu_cases())
def test_every_gpu_case_is_certified(P, family):
    case = C.make_case(P, family, SEED)
    bits = C.certificate(case)
    f = C.FAMILIES[family]
    assert max(bits.values()) <= C.closed_form_bits(P, f["md"], f["ma"]) < 24.0
    print("\n%s P=%d: worst %.2f bits (%s)" % (family, P, max(bits.values()), max(bits, key=bits.get)))


@pytest.mark.parametrize("P", PLAN_P)
@pytest.mark.parametrize("family", ["narrow", "narrow_signed"])
def test_large_sizes_are_certified_in_closed_form(P, family):
    f = C.FAMILIES[family]
    assert P <= f["max_P"] and C.closed_form_bits(P, f["md"], f["ma"]) < 24.0
    case = C.make_case(300, family, SEED)                      # the construction keeps the family's magnitudes (any P: the marks are the largest values)
    assert max(float(d.abs().max()) for d in case["deltas"] + [case["d_rgb"], case["d_sig"]]) == f["md"]
    assert max(float(a.abs().max()) for a in case["acts"] + [case["x"]]) == f["ma"]


def test_wide_families_stop_where_the_bound_stops():
    for name, f in C.FAMILIES.items():
        assert C.closed_form_bits(f["max_P"], f["md"], f["ma"]) < 24.0, name
        if name.startswith("wide"):
            bd, ba = f["md"].bit_length(), f["ma"].bit_length()
            assert bd + ba + (f["max_P"] - 1).bit_length() == 24, name       # b_d + b_a + ceil(log2 P) <= 24, with nothing to spare


@pytest.mark.parametrize("family", ["narrow", "narrow_signed", "wide_6_11"])
def test_fp32_numpy_in_any_order_gives_the_reference_to_the_bit(family):
    P = 128 if family == "wide_6_11" else 1025
    case = C.make_case(P, family, SEED)
    ref = dict(zip(C.TENSOR_NAMES, C.reference(case)))
    jobs = {name: (D, blocks) for name, D, blocks in C.jobs(case)}
    rng = np.random.default_rng(5)
    for name in ("xyz_encoding_1.0", "xyz_encoding_5.0", "static_rgb.0"):
        D, blocks = jobs[name]
        A = torch.cat(blocks, 1)
        want = ref[name + ".weight"].numpy()
        for order in (rng.permutation(P), rng.permutation(P)):
            for chunk in (128, 37):
                got = C.numpy_chunked(D, A, order, chunk)
                assert got.dtype == np.float32 and np.array_equal(got.astype(np.float64), want), (name, chunk)
        assert np.array_equal(D.numpy()[rng.permutation(P)].sum(0, dtype=np.float32).astype(np.float64), ref[name + ".bias"].numpy()), name


def test_a_case_beyond_the_bound_fails_the_certificate():
    case = C.make_case(2049, "narrow", SEED)
    C.certificate(case)
    case["x"][:, 5] = 8191.0                                   # a 13-bit input column against a delta column of 2s: 2 * 8191 * 2049 > 2^24
    case["deltas"][0][:, 7] = 2.0
    with pytest.raises(AssertionError, match="xyz_encoding_1.0 needs"):
        C.certificate(case)
    assert C.closed_form_bits(2 ** 18, 2, 8191) >= 24.0        # and in closed form at the large sizes


@pytest.mark.parametrize("P", [1, 33, 300])
def test_pack_and_unpack_round_trip(P):
    case = C.make_case(P, "narrow_signed", SEED)
    L = C.layout(P)
    dwords, aword = C.true_words(case)
    acts, scratch = C.pack_state(case, L["acts_min"], L["ws"] + 4096, dwords, aword)
    assert acts.numel() == L["acts_min"] and scratch.numel() == L["ws"] + 4096
    back = C.unpack_state(case["x"], acts, scratch, P)
    for k in ("x", "d_rgb", "d_sig"):
        assert torch.equal(back[k], case[k]), k
    for k in ("acts", "deltas"):
        assert all(torch.equal(a, b) for a, b in zip(back[k], case[k])), k
    assert back["dmax_words"] == dwords + [0] * (C.RANGE_WORDS - C.RANGE_USED) and back["amax_word"] == aword
    acts2, scratch2 = C.pack_state(back, acts.numel(), scratch.numel(), back["dmax_words"], back["amax_word"])
    assert torch.equal(acts2, acts) and torch.equal(scratch2, scratch)
    # the documented places, spelled out once more: slot s, point p, column c of the activations / deltas; d_rgb, d_sig, the words
    f = lambda buf, byte: float(buf[byte:byte + 4].view(torch.float32)[0])   # noqa: E731
    s, p, c = 9, P - 1, 255
    assert f(acts, ((s * P + p) * 256 + c) * 4) == float(case["acts"][s][p, c])
    assert f(scratch, ((s * P + p) * 256 + c) * 4) == float(case["deltas"][s][p, c])
    assert f(scratch, 10 * P * 1024 + (p * 64 + 63) * 4) == float(case["d_rgb"][p, 63])
    assert f(scratch, 10 * P * 1024 + P * 256 + p * 4) == float(case["d_sig"][p])
    assert f(scratch, 10 * P * 1024 + P * 256 + P * 4 + 10 * 4) == float(case["d_rgb"].abs().max())
    assert f(acts, 10 * P * 1024 + 10 * P * 32) == 15.0
    assert not bool(acts[10 * P * 1024:10 * P * 1024 + 10 * P * 32].any())          # the relu bits stay zero


def test_the_edge_marks_are_where_the_docstring_says():
    for family, f in C.FAMILIES.items():
        P = min(300, f["max_P"])
        case = C.make_case(P, family, SEED)
        for t, m in [(case["x"], f["ma"]), (case["d_rgb"], f["md"])] + [(a, f["ma"]) for a in case["acts"]] + [(d, f["md"]) for d in case["deltas"]]:
            assert bool((t[P - 1] != 0).all()), family                                              # every column is non-zero somewhere
            assert bool((t[P - 1, 1:] != t[P - 1, :-1]).all()), family                              # each column differs from its neighbours
            if m >= 2:                                                                              # values no other point has in that column
                assert not bool((t[:P - 1] == t[P - 1]).any()), family
                blocks = t[127:P - 1:128]
                rest = torch.ones(P, dtype=torch.bool)
                rest[127::128] = False
                rest[P - 1] = False
                assert blocks.numel() == 0 or not bool((t[rest][:, None, :] == blocks[None]).any()), family
            assert 0.3 < float((t == 0).float().mean()) < 0.7 or P < 16, family


@pytest.mark.parametrize("family", list(C.FAMILIES))
def test_mode_lists_obey_the_piece_rules(family):
    f = C.FAMILIES[family]
    for P in sorted({1, min(33, f["max_P"]), f["max_P"] if f["max_P"] <= 128 else 129}):
        fair = C.fair_modes(C.make_case(P, family, SEED))
        assert set(f["modes"]) <= set(fair), (family, P, fair)
        assert "fp32" in fair
    if family.startswith("wide"):
        assert "bf16" not in C.fair_modes(C.make_case(f["max_P"], family, SEED))       # more than 8 significant bits somewhere
    # the rules bite: 18-bit operands on BOTH sides lose piece products in both split modes
    both = C.make_case(16, "wide_1_18", SEED)
    both["deltas"] = C.make_case(16, "wide_18_1", SEED)["deltas"]
    assert C.fair_modes(both) == ("fp32",)
    # and a tensor whose values span more than fp16's exponent range under one scale has no exact fp16 pieces
    spread = C.make_case(16, "narrow", SEED)
    spread["acts"][0][0, 0] = 2.0 ** 30
    assert "f16x2" not in C.fair_modes(spread)


def test_which_families_reach_second_and_third_pieces():
    """17-bit integers fit two round-to-nearest bf16 pieces (the second piece is signed); 18 bits reach the third.  Both reach second fp16 pieces."""
    for family, third in (("wide_1_17", False), ("wide_17_1", False), ("wide_1_18", True), ("wide_18_1", True), ("wide_6_11", False)):
        f = C.FAMILIES[family]
        case = C.make_case(f["max_P"], family, SEED)
        wide = case["acts"][3] if f["ma"] > f["md"] else case["deltas"][3]
        (w1, w2, w3), exact = C.pieces_bf16(wide)
        assert exact and bool(w2.any()) and bool(w3.any()) == third, family
        word = C.range_word(wide)
        (h1, h2), hexact, sub = C.pieces_f16(wide, C.act_scale(word) if f["ma"] > f["md"] else C.delta_scale(word))
        assert hexact and not sub and bool(h2.any()) == (family != "wide_6_11"), family

"""CPU half of the bit-exact encoder tests (tests/_encoder_cases.py holds the construction and its reasoning): the certificate that makes every
summation order exact holds for every case; the fp32 CPU oracle, in two summation orders, already equals the float64 one bit for bit on them;
and the sparse inputs have teeth -- a numpy emulation of the kernels' index arithmetic reproduces the float64 reference exactly, and each of five
single-line index errors in it changes the expected bits of some case.  tests/test_gpu_encoder_exact.py then holds the HIP kernels to the same
expected values with torch.equal.

CRNERF_ENCODER_EXACT_OUT=<file>: the certificate margins and the mutant / case table are also written there (profiles/r9/encoder_exact.txt)."""
import os

import numpy as np
import pytest
import torch

import _encoder_cases as E
from crnerf_amd.parallel import encoder_band_plan

_report = {"margins": {}, "mutants": {}}


def _flush_report():
    path = os.environ.get("CRNERF_ENCODER_EXACT_OUT")
    if not path:
        return
    lines = ["Exactly summable encoder cases (tests/_encoder_cases.py): certificate margins and what the cases can see",
             "",
             "1. certificate(case): worst log2(sum|terms| / quantum) over every sum of a kind; every order is exact in fp32 below 24",
             "   columns: forward sums (conv1..7, avgpool) | bias gradients | weight gradients | data gradients (conv7..1, avgpool backward)", ""]
    for name, bits in _report["margins"].items():
        kind = lambda s: max([v for k, v in bits.items() if s in k] or [float("-inf")])   # noqa: E731
        lines.append("%-22s forward %5.1f | bias gradient %5.1f | weight gradient %5.1f | data gradient %5.1f | worst %5.1f  (%s)"
                     % (name, max(kind("forward"), kind("avgpool forward")), kind("bias gradient"), kind("weight gradient"),
                        max(kind("data gradient"), kind("avgpool backward")), max(bits.values()), max(bits, key=bits.get)))
    if _report["mutants"]:
        lines += ["", "2. index-arithmetic mutants (Emulation(mutant) in tests/_encoder_cases.py) against the float64 reference, per case:",
                  "   the outputs whose bits change ('-': the case cannot see this mutant; 'out' = the forward output)", ""]
        for m in E.MUTANTS:
            lines.append(m)
            for name, bad in _report["mutants"].get(m, {}).items():
                lines.append("    %-14s %s" % (name, "-" if not bad else "%d of 16: %s" % (len(bad), " ".join(b.replace("conv", "c").replace(".weight", "w").replace(".bias", "b") for b in bad))))
        lines += ["", "clamp_early: " + E.Emulation.clamp_note]
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


@pytest.fixture(scope="module", autouse=True)
def _write_report():
    yield
    _flush_report()


def test_first_maximum_is_atens_tie_rule():
    assert E.first_maximum_rule_holds()


@pytest.mark.parametrize("name", E.CASE_NAMES)
def test_certificate_holds(name):
    case = E.get_case(name)
    bits = E.certificate(case)
    _report["margins"][name] = bits
    print("\n%s: " % name + ", ".join("%s %.1f" % kv for kv in bits.items()))
    assert len(bits) == 8 + 7 * 3 + 1 and max(bits.values()) < 24.0
    for t in [case["img"], case["cot"]] + list(case["weights"].values()):      # the inputs themselves are fp32 numbers
        assert np.array_equal(t.astype(np.float32).astype(np.float64), t)
    assert (case["img"] >= 0).all() and all((v >= 0).all() for v in case["weights"].values())
    assert all((case["weights"]["conv%d.bias" % i] > 0).all() for i in range(1, 8))
    sc, want = E.sign_case(case)
    fwd = E.certificate(sc, forward_only=True)
    _report["margins"][name + " (sign)"] = fwd
    assert max(fwd.values()) < 24.0 and 0.25 < float((want < 0).mean()) < 0.75


@pytest.mark.parametrize("name,ws", E.BAND_CASES)
def test_certificate_holds_for_row_bands(name, ws):
    """A band's backward = the whole image's with the cotangent restricted to the band's rows of the 32 x 32 grid (what lies outside its halo gets
    no gradient from them); its forward runs on the band's rows as an image of their own, whose cut edges reflect other values: both are covered."""
    case = E.get_case(name)
    for rank in range(ws):
        _, row0, rows, o0, o1, _ = encoder_band_plan(case["H"], case["W"], ws, rank)
        bits = E.certificate(case, rows=(o0, o1))
        sub = dict(case, img=case["img"][:, row0:row0 + rows], H=rows, name="%s rows %d..%d" % (name, row0, row0 + rows))
        bits.update({"band " + k: v for k, v in E.certificate(sub, forward_only="conv6").items()})
        _report["margins"]["%s band %d/%d" % (name, rank, ws)] = bits
        assert max(bits.values()) < 24.0
        ref = E.reference(case, bands=[(o0, o1)])["bands"][0]
        outside = torch.cat((ref["d_img"][:, :row0], ref["d_img"][:, row0 + rows:]), dim=1)
        assert not outside.any(), "the band's output rows reach image rows outside its halo"


@pytest.mark.parametrize("name", E.CASE_NAMES)
def test_fp32_oracle_equals_float64_in_two_summation_orders(name):
    case = E.get_case(name)
    ref = E.reference(case)
    assert not E.differs(ref, E.reference(case, forward=E.encoder_forward_im2col)), "the float64 restatements disagree"
    for forward in (E.O.encoder_forward, E.encoder_forward_im2col):
        got = E.reference(case, dtype=torch.float32, forward=forward)
        cast = {"out": got["out"].double(), "grads": [g.double() for g in got["grads"]], "d_img": got["d_img"].double()}
        assert not E.differs(ref, cast), (forward.__name__, E.differs(ref, cast))


_EMULATED = [n for n in E.CASE_NAMES if n != "130x128"]      # (the mutants run where a run takes well under a second)


@pytest.mark.parametrize("name", E.CASE_NAMES)
def test_index_emulation_equals_the_reference(name):
    case = E.get_case(name)
    assert not E.differs(E.reference(case), E.Emulation().run(case))


@pytest.mark.parametrize("mutant", E.MUTANTS)
def test_every_index_mutant_changes_some_case(mutant):
    """The power check: were the sparse dyadic inputs blind to an index error, bit equality on the GPU would prove little."""
    seen = {}
    for name in _EMULATED:
        case = E.get_case(name)
        seen[name] = E.differs(E.reference(case), E.Emulation(mutant).run(case))
    _report["mutants"][mutant] = seen
    print("\n%s: " % mutant + ", ".join("%s %d" % (n, len(b)) for n, b in seen.items()))
    assert any(seen.values()), "no case sees " + mutant
    if mutant == "floor_window_end":            # windows that end on a grid line (H4 = 32, 64) are the same either way; H4 < 32 loses whole windows
        assert seen["192x8"] and not seen["256x16"] and not seen["128x24"]
    if mutant in ("reflect_high", "drop_row_n_minus_2", "last_maximum"):
        assert sum(bool(b) for b in seen.values()) >= len(seen) // 2, seen


def test_all_cases_together_touch_every_tap():
    used = {i: np.zeros(E.CIN[i - 1] * E.TAPS[i - 1], dtype=bool) for i in range(1, 8)}
    rows = {i: np.zeros(E.COUT[i - 1], dtype=bool) for i in range(1, 8)}
    for name in E.CASE_NAMES:
        for i in range(1, 8):
            m = E.get_case(name)["weights"]["conv%d.weight" % i].reshape(E.COUT[i - 1], -1) != 0
            used[i] |= m.any(axis=0)
            rows[i] |= m.any(axis=1)
    for i in range(1, 8):
        assert used[i].all(), "conv%d: (channel, tap) columns %s are zero in every case" % (i, np.flatnonzero(~used[i]).tolist())
        assert rows[i].all()
    assert sorted({E.get_case(n)["dense"] for n in E.CASE_NAMES}) == [2, 3, 4, 5, 6, 7]

"""No GPU: the fp32 CPU oracle's sample_pdf and compositing against their float64 evaluations on the inputs of tests/test_gpu_ray_edges.py
(tests/_ray_cases.py).  Shows that these inputs are ones on which the reference alone meets the bounds the kernels are then held to, and
supplies the measured constants those bounds are built from (printed: run with -s to read them)."""
import pytest
import torch

import _ray_cases as RC
from oracle import cpu_ref as O


@pytest.mark.parametrize("family", RC.FAMILIES)
def test_fp32_oracle_sample_pdf_vs_float64(family):
    """Every (family, shape) keeps >= 95 % of its samples pinned, and the fp32 oracle meets the pinned bound with K_ORACLE there."""
    k_needed, max_err = 0.0, 0.0
    for nc, ni in RC.SHAPES:
        zc, w, u = RC.sample_case(family, nc, ni)
        z32 = O.sample_pdf(RC.midpoints(zc), w[:, 1:-1], ni, u=u)
        assert z32.dtype == torch.float32
        st = RC.check_samples(z32, zc, w, u, RC.K_ORACLE, min_share=RC.MIN_PINNED_SHARE, what="%s (%d, %d)" % (family, nc, ni))
        print("sample_pdf %-8s (%3d, %3d): pinned share %.3f, K needed %.3f, largest pinned error %.3g" % (family, nc, ni, st["share"], st["k_needed"],
                                                                                                    st["max_err"]))
        k_needed, max_err = max(k_needed, st["k_needed"]), max(max_err, st["max_err"])
    print("sample_pdf %-8s: measured K %.3f (K_ORACLE %.2f, K_KERNEL %.2f), largest pinned error %.3g" % (family, k_needed, RC.K_ORACLE, RC.K_KERNEL, max_err))


def test_measured_k_is_the_recorded_one():
    """K_ORACLE is the measured constant rounded up, not a number with room in it: the oracle needs more than half of it somewhere."""
    worst = 0.0
    for family in RC.FAMILIES:
        for nc, ni in RC.SHAPES:
            zc, w, u = RC.sample_case(family, nc, ni)
            worst = max(worst, RC.check_samples(O.sample_pdf(RC.midpoints(zc), w[:, 1:-1], ni, u=u), zc, w, u, RC.K_ORACLE)["k_needed"])
    assert 0.5 * RC.K_ORACLE < worst <= RC.K_ORACLE, worst


def test_families_are_what_they_claim():
    zc, w, _ = RC.sample_case("blocks", 256, 256)
    inner = w[:, 1:-1].double()
    assert 0.35 < float((inner == 0).double().mean()) < 0.65
    assert float((inner.sum(1) - 4).abs().max()) < 1e-5
    pdf = (inner + 1e-5) / (inner + 1e-5).sum(1, keepdim=True)
    assert float(pdf[inner == 0].max()) <= 2.6e-6 and float(pdf[inner > 0].min()) >= 1e-3
    assert bool((RC.sample_case("zero", 67, 129)[1][:, 1:-1] == 0).all())
    one = RC.sample_case("onehot", 67, 129)[1][:, 1:-1]
    assert bool((one.sum(1) == 1).all()) and bool((one.max(1)[0] == 1).all())
    assert bool((zc[:, 1:] > zc[:, :-1]).all())
    g = RC.generator(1, 2, 3)
    zt = RC.tied_depths(8, 130, g)
    same = zt[:, 1:] == zt[:, :-1]
    assert bool((zt[:, 1:] >= zt[:, :-1]).all()) and 0.5 < float(same.double().mean()) < 0.85
    run = torch.zeros(8, dtype=torch.long)
    longest = 0
    for j in range(129):
        run = torch.where(same[:, j], run + 1, torch.zeros_like(run))
        longest = max(longest, int(run.max()))
    assert longest == 4          # runs of at most 5 equal depths


@pytest.mark.parametrize("kind", RC.COMPOSITE_KINDS)
def test_fp32_oracle_composite_vs_float64(kind):
    worst = {k: 0.0 for k in RC.FLOORS}
    for n in RC.COMPOSITE_N:
        case = RC.composite_case(kind, n)
        ref, got = RC.composite_ref64(case), RC.composite_oracle32(case)
        for k in worst:
            worst[k] = max(worst[k], float((got[k].double() - ref[k]).abs().max()))
        # what the kind promises holds in the reference itself
        assert bool((ref["weights"][case["zero_weight"]] == 0).all()) and bool((got["weights"][case["zero_weight"]] == 0).all())
        if kind == "saturated":
            assert float((ref["weights"].sum(1) - 1).abs().max()) <= 1e-6
        if kind == "clamped" and n >= 31:
            eff = case["raw"][..., 64] + case["noise"] * case["noise_std"]
            assert bool((eff == 0).any(1).all()) and 0.35 < float((eff <= 0).double().mean()) < 0.75
        if kind == "thin" and n == 257:
            z, sigma = case["z"].double(), case["raw"][..., 64].double()
            alpha = 1 - torch.exp(-(z[:, 1:] - z[:, :-1]) * sigma[:, :-1])
            assert 2e-5 < float(alpha.min()) and float(alpha.max()) < 4e-4
            assert float((ref["weights"][:, -2] / alpha[:, -1]).min()) > 0.9       # T after 255 samples: still most of the light
        if kind == "empty":
            assert bool((ref["feature"] == 0).all()) and bool((ref["depth"] == 0).all())
    tol = RC.composite_tolerances(kind)
    print("composite %-9s: fp32 oracle vs float64 %s -> kernel tolerance %s" % (kind, {k: "%.3g" % v for k, v in worst.items()},
                                                                               {k: "%.3g" % v for k, v in tol.items()}))
    for k in worst:
        assert worst[k] <= RC.COMPOSITE_ORACLE_ERR[kind][k], (k, worst[k])


@pytest.mark.parametrize("kind", RC.COMPOSITE_KINDS)
def test_fp32_oracle_composite_backward_vs_float64(kind):
    worst = 0.0
    for n in RC.COMPOSITE_BACKWARD_N:
        case = RC.composite_case(kind, n)
        ref, got = RC.composite_backward_ref(case), RC.composite_backward_ref(case, torch.float32)
        worst = max(worst, float((got.double() - ref).abs().max()) / (float(ref.abs().max()) + 1e-6))
        ds64, ds32 = ref[..., 64][case["zero_dsigma"]], got[..., 64][case["zero_dsigma"]]
        # autograd multiplies by exp(-delta * sigma), which at sigma = 1e4 is 1e-35 or less but not always 0; the kernel multiplies by the
        # 1 - alpha it composited with, which is exactly 0
        assert bool((ds32.abs() <= 1e-30).all()) and bool((ds64.abs() <= 1e-30).all())
        if kind != "saturated":
            assert bool((ds32 == 0).all()) and bool((ds64 == 0).all())
    print("composite backward %-9s: fp32 autograd vs float64 %.3g of max |gradient| -> kernel tolerance %.3g" %
          (kind, worst, max(2 * RC.COMPOSITE_BACKWARD_ORACLE_ERR[kind], RC.BACKWARD_FLOOR)))
    assert worst <= RC.COMPOSITE_BACKWARD_ORACLE_ERR[kind], worst

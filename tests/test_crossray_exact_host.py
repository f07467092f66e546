"""CPU half of the bit-exact tests of the cross-ray decoder (tests/_crossray_cases.py holds the constructions and their reasoning): every case that
tests/test_gpu_crossray_exact.py uses passes its certificate here too, a case beyond a bound is refused, the integer references are tied to
oracle.cpu_ref.crossray_decode in float64 through the stage-by-stage composition, and the tolerance-based checks are certified to SEE: the
derived bound of the matrix stage against a one-row shift of fc_w, the whole-decode bar against three slips of the statistics, the per-element
check of d_content against the part that flows through the Gram chains, tile by tile."""
import numpy as np
import pytest
import torch

import _crossray_cases as C

from _crossray_cases import (APPLY_HW, BACKWARD, CHANSUM_HW, DECODE, GRAM_HW, GRAM_SEEDS, MATRIX_COUNTS, TWO_JOB, style_mean)


# ------------------------------------------------------------------------------------------------------------------ certificates
def test_every_gpu_case_is_certified():
    lines = ["chansum %d: %.2f bits" % (HW, C.chansum_case(HW)["bits"]) for HW in CHANSUM_HW]
    for seed in GRAM_SEEDS:
        for HW in GRAM_HW:
            c = C.gram_case(HW, seed)
            lines.append("gram seed %d HW %d: %.2f bits, branches (+, -) %s" % (seed, HW, c["bits"], c["branches"]))
    for HW, HWs in TWO_JOB:
        c, s = C.gram_case(HW, 2), C.gram_case(HWs, 3, style_mean(HWs))
        assert style_mean(HWs) == "int" or not s["sums"].any()
        lines.append("two jobs (%d, %d): %.2f / %.2f bits" % (HW, HWs, c["bits"], s["bits"]))
    lines += ["matrix count %d: %.2f bits" % (n, C.matrix_case(n)["bits"]) for n in MATRIX_COUNTS]
    lines.append("fold: %.2f bits" % C.fold_case()["bits"])
    for HW in APPLY_HW:
        C.apply_case(HW)
    print("\n" + "\n".join(lines))


def test_a_case_beyond_a_bound_is_refused(monkeypatch):
    with pytest.raises(AssertionError, match="multiple of 5"):
        C.lrelu_int(np.array([-25, -7]))
    w = C.cnn_weights(0)
    with pytest.raises(AssertionError, match="multiple of 25"):
        C.chain_int(np.full((3, 64), 5, np.int64), w)
    C.gram_case(4097, 0)
    monkeypatch.setattr(C, "LIMIT", 1 << 19)                     # the 4,097-pixel case needs 19.8 bits
    with pytest.raises(AssertionError, match="Gram: sum"):
        C.gram_case(4097, 0)
    with pytest.raises(AssertionError, match="quanta"):
        C.matrix_case(1024)
    w[5][:] = 0                                                  # no b3, no bias anywhere: a pixel with x = mean has h3 = 0
    w[1][:] = 0
    w[3][:] = 0
    _, _, h3 = C.chain_int(np.zeros((2, 64), np.int64), w)
    assert not h3.any()


def test_lrelu_in_fp32_is_a_division_by_five_on_multiples_of_five_only():
    v = -5 * np.arange(1, 200001, dtype=np.int64)
    assert (np.float32(0.2) * v.astype(np.float32) == (v // 5).astype(np.float32)).all()
    odd = np.float32(0.2) * np.float32(-7.0)
    assert float(odd) != -1.4 and float(odd) != round(float(odd))


# ------------------------------------------------------------------------------------------------------------------ the references' tie to the oracle
def test_the_integer_references_compose_to_the_float64_oracle():
    """One exact case per stage, chained: integer channel sums -> means, int64 Gram sums of both chains, the matrix and fold references on them,
    sigmoid in float64 -- against oracle.cpu_ref.crossray_decode in float64 on the same grids and weights."""
    from oracle import cpu_ref as O
    import crnerf_amd.synth as synth
    cg, sg = C.gram_case(129, 1), C.gram_case(64, 0)
    rng = np.random.default_rng(5)
    fold = C.fold_case(1)
    fc = [C.sparse_int(rng, 1024, 1024, np.full(1024, 3), [-1, 1]).astype(np.float64) * 2.0 ** -12 for _ in range(2)]
    fb = [rng.integers(-2, 3, 1024).astype(np.float64) for _ in range(2)]
    weights = [t.astype(np.float64) for t in sg["w"]] + [fc[0], fb[0]] + [t.astype(np.float64) for t in cg["w"]] + [fc[1], fb[1]]
    weights += [t.astype(np.float64) for t in fold["lin"]]
    # a power of two on the rgb conv that brings the image out of saturation (|pre-activation| <= 4)
    aff = C.ref_fold(C.ref_matrix(sg["want"], 64, fc[0], fb[0]), C.ref_matrix(cg["want"], 129, fc[1], fb[1]), cg["mean"].astype(np.float64),
                     sg["mean"].astype(np.float64), weights[16:22])
    pre = np.abs(aff[:192].reshape(3, 64) @ cg["x"].astype(np.float64).T + aff[192:, None]).max()
    weights[20], weights[21] = weights[20] * 2.0 ** -np.ceil(np.log2(pre / 4)), weights[21] * 2.0 ** -np.ceil(np.log2(pre / 4))
    # by the stage references
    c_sum, s_sum = cg["x"].astype(np.int64).sum(0), sg["x"].astype(np.int64).sum(0)
    assert np.array_equal(c_sum / 129.0, cg["mean"]) and np.array_equal(s_sum / 64.0, sg["mean"])
    sM = C.ref_matrix(sg["want"], 64, fc[0], fb[0])
    cM = C.ref_matrix(cg["want"], 129, fc[1], fb[1])
    rgb = C.ref_apply(cg["x"], C.ref_fold(sM, cM, cg["mean"].astype(np.float64), sg["mean"].astype(np.float64), weights[16:22]))
    # by the oracle
    st = {k: torch.from_numpy(np.ascontiguousarray(w).reshape(synth.DECODER_SHAPES[k])) for k, w in zip(C.weight_names(), weights)}
    x, s = torch.from_numpy(cg["x"]).double(), torch.from_numpy(sg["x"]).double()
    ref = O.crossray_decode(st, O.feature_to_grid(x, 1, 129), O.feature_to_grid(s, 1, 64)).reshape(3, -1).numpy()
    assert 0.01 < ref.min() and ref.max() < 0.99 and ref.std() > 0.01           # an image, not a saturated constant
    np.testing.assert_allclose(rgb, ref, rtol=1e-12, atol=0)
    # and the float64 stage composition used for the sensitivity certificates is the same function
    mine = C.stages64(cg["x"], sg["x"], weights)
    np.testing.assert_allclose(mine["rgb"], ref, rtol=1e-12, atol=0)
    assert np.array_equal(mine["c_gram"], cg["want"]) and np.array_equal(mine["s_gram"], sg["want"]) and np.array_equal(mine["c_sum"], c_sum)


def test_decode_torch_is_the_oracle():
    from oracle import cpu_ref as O
    case = C.backward_case(33, 64)
    w = {k: torch.from_numpy(v).double() for k, v in case["state"].items()}
    x, s = torch.from_numpy(case["content"]).double(), torch.from_numpy(case["style"]).double()
    ref = O.crossray_decode(w, O.feature_to_grid(x, 1, 33), O.feature_to_grid(s, 1, 64)).reshape(3, -1)
    for detach in (False, True, "matrices"):
        assert torch.equal(C.decode_torch(w, x, s, detach), ref)


# ------------------------------------------------------------------------------------------------------------------ the bars see
@pytest.mark.parametrize("count", [1000, 4097])
def test_the_matrix_bound_sees_a_one_row_shift(count):
    c = C.matrix_case_dense(count)
    shifted = C.ref_matrix(c["g"], count, np.roll(c["w"], 1, axis=0), c["b"])
    ratio = np.abs(shifted - c["want"]) / c["bound"]
    print("\ncount %d: a one-row shift of fc_w moves the rows by %.0f x the bound (median), %.1f %% of the rows by 10 x or more"
          % (count, np.median(ratio), 100 * (ratio >= 10).mean()))
    assert np.median(ratio) >= 100 and (ratio >= 10).mean() >= 0.95
    # the fp32 evaluation in the kernel's own order sits inside the bound
    inv = np.float32(1.0 / count)
    mine = ((c["w"] * (c["g"] * inv)[None, :]).astype(np.float32).sum(1, dtype=np.float32) + c["b"]).astype(np.float64)
    assert (np.abs(mine - c["want"]) <= c["bound"]).all()


@pytest.mark.parametrize("HW,HWs", DECODE)
def test_the_decode_bar_sees_three_slips_of_the_statistics(HW, HWs):
    case = C.decode_case(HW, HWs)
    ref, own, bar = C.decode_reference(case)
    assert bar == max(2e-5, 4 * own)
    base = C.stages64(case["content"], case["style"], case["weights"])["rgb"]
    np.testing.assert_allclose(base, ref, rtol=1e-10, atol=1e-13)
    assert ref.std() > 0.1                                      # an image with contrast
    moved = {}
    for slip in ("swap_matrices", "swap_means", "style_count"):
        if slip == "style_count" and HW == HWs:
            continue                                            # equal counts: dividing by the other grid's count is no slip
        moved[slip] = float(np.abs(C.stages64(case["content"], case["style"], case["weights"], slip)["rgb"] - ref).max()) / bar
        assert moved[slip] >= 100, (slip, moved[slip])
    print("\n(%d, %d): fp32 CPU oracle %.2e from float64, bar %.1e; slips move a pixel by %s x the bar"
          % (HW, HWs, own, bar, ", ".join("%s %.0f" % kv for kv in moved.items())))


@pytest.mark.parametrize("HW,HWs", BACKWARD)
def test_backward_cases_sit_off_the_lrelu_kinks(HW, HWs):
    """The gradient of lrelu jumps at 0, so a backward case is only as good as its distance from the kinks: every pre-activation of both
    chains is further from 0 than any fp32 evaluation can be from float64 (_crossray_cases.kink_margin), while the uniform grids the case
    was made from are not."""
    raw = C.decode_case(HW, HWs, 13)
    before, on_kink = C.kink_margin(raw["content"], raw["weights"][8:12])
    case = C.backward_case(HW, HWs)
    print("\n(%d, %d): margin %.3f with %d content pixels on a kink before, %.2f after" % (HW, HWs, before, len(on_kink), case["kink_margin"]))
    assert before < 1.0 and case["kink_margin"] > 1.0
    assert np.allclose(case["content"].astype(np.float64).mean(0), raw["content"].astype(np.float64).mean(0), rtol=0, atol=1e-8)     # the means stay


@pytest.mark.parametrize("HW,HWs", BACKWARD)
def test_every_tile_of_d_content_sees_its_gram_part(HW, HWs):
    case = C.backward_case(HW, HWs)
    part, bar = C.tile_gram_part(case)
    chain, _ = C.tile_gram_part(case, "matrices")
    print("\n(%d, %d): in every 32-pixel tile the Gram part of d_content is >= %.0f x the bar, the conv chains' own share >= %.1f x"
          % (HW, HWs, part.min() / bar, chain.min() / bar))
    assert part.min() >= 10 * bar
    assert chain.min() >= 2 * bar                               # a tile whose chain gradient is lost or zero errs by this much
    # the cnet conv gradients are chain deltas and nothing else: a chain that is wrong as a whole cannot hide behind the direct path
    grads = C.backward_reference(case, detach_stats="matrices")[2]
    assert all(not grads[k].any() for k in C.weight_names()[8:14]) and all(np.abs(g).max() > 0 for g in C.backward_reference(case)[2].values())


def test_a_planar_out_view_may_have_its_own_plane_stride_and_nothing_else():
    from crnerf_amd import ops
    like = torch.zeros(4, 64)
    buf = torch.zeros(3, 9)
    view = buf[:, :4]
    assert ops._planar_out(view, 4, like) is view and ops._planar_out(None, 4, like).shape == (3, 4)
    for bad in (torch.zeros(4, 3).t(), buf[:, :5], buf[:, :4].double(), torch.zeros(3, 8)[:, ::2]):
        with pytest.raises(ValueError, match="dense planes"):
            ops._planar_out(bad, 4, like)

"""The cross-ray decoder (csrc/crossray.hip) stage by stage on the device, its sums BIT FOR BIT, past every size at which it changes its code
path.  tests/_crossray_cases.py holds the constructions, the certificates and the references; tests/test_crossray_exact_host.py runs the same
certificates on the CPU, ties the references to oracle.cpu_ref.crossray_decode in float64 and certifies that the tolerance-based checks below see
what they are for.

1. ops.crossray_chansum, crossray_gram, crossray_matrix, crossray_fold on inputs for which every fp32 summation order is exact, torch.equal
   against int64: one tile per workgroup against one per wave (4,096 / 4,097 pixels), the second trip of the tile loop (32,769), `per` = 2
   with empty trailing workgroups (16,385), the second eight-stream pass (131,073); the two-job Gram launch with the mean taken from sums, in
   all four cooperative / non-cooperative pairings -- the style job's mean and Gram are read from the workspace where the backward reads them
   (_crossray_cases.WS_STATS); crossray_matrix with a count that is no power of two against float64 inside a derived, order-independent bound;
   crossray_apply on integer pre-activations (equal pre-activations -> equal bits) into a strided view whose pad columns must stay NaN, past the
   2,048-workgroup cap of its grid.
2. The whole decode, ops.crossray_decode and the five stage calls composed by hand, through synth.decoder_state(contrast=4000) -- the decoder that
   sees: with default-contrast weights a feature error is damped ~500 x -- against float64 at max(2e-5, 4 x the fp32 CPU oracle's own error).
3. The backward past its switches (forward re-run on the six-launch path, the chain kernel's 256-workgroup cap, its capped channel sums): one rank
   emulated through the three phases of ops.crossray_decode_backward_sharded on a caller-built state whose workspace (exactly the library's byte
   count), d_content, d_style and 22 gradient tensors are filled with 0xff bytes -- NaN --, and once through ops.crossray_decode_backward, against
   float64 autograd through the oracle at the bar of test_decoder_backward_vs_autograd_oracle.  d_content is checked per element, and every
   32-pixel tile of it carries a Gram part of >= 150 x the bar (host test).  A tile lost by the chain kernel is diluted by 1 / n in the
   parameter gradients: for those the NaN poison is the instrument -- a tile the kernel skips, a partial row nobody wrote, a pad lane read as
   data surface as NaN in the sums.  d_rgb is N(3, 1): see _crossray_cases.D_RGB_MEAN for why a zero-mean d_rgb cannot work.  The grids are moved
   off the lrelu kinks (_crossray_cases.off_the_kinks, certified on the host): lrelu's gradient jumps at 0, and on a plain uniform grid of
   32,801 pixels half an fp32 ulp on the mean flips one of some twenty pre-activations within 1e-6 of 0 -- the first run of this file showed
   the two entry points 1.5e-3 (d_content) and 2.6e-4 (first conv weight gradient) of a tensor's maximum apart for that reason alone.

MEASURED on an MI355X (256 compute units) when these tests were written: every bit-for-bit test passes at every size -- no kernel of the forward
was found to differ from its reference; crossray_matrix with counts 1,000 / 4,097 errs by less than 0.0005 of its bound; crossray_apply is 5.5e-8
from float64 sigmoid (bar 1e-6); the whole decode is 7.7e-7 ... 1.2e-6 from float64 in one call and 7.3e-7 ... 1.0e-6 by hand (bar 2e-5; the fp32
CPU oracle's own error 5.3e-7 ... 9.8e-7); the backward is finite on poisoned memory, its worst tensor (compress.weight) 2.6e-6 ... 5.2e-6 of
max|ref| from float64 (bar 2e-3), d_content 7.9e-7 ... 1.5e-6, and the two entry points 0 ... 6.3e-6 apart (bar 3e-5).  The whole file takes 7 s, the
largest test 0.7 s.  Mutation check (scratch builds of csrc/crossray.hip, one value-only line each; "old" = the 19 decoder tests of test_gpu_parity.py,
test_gpu_train_aux.py and test_gpu_e2e_parity.py):
  lrelu02 slope 0.25                                  red here (49: Gram 26, two-job 5, decode 10, backward 8); old: 11 red
  gram_tiles: `valid` forced true in the transpose    red here (24: Gram 6, two-job 4, decode 8, backward 6); old: 1 red (the 100 x 100 ragged grid)
  gram_tiles_coop: the same                           red here (19); old: 5 red
  gram_fc_small_kernel: the other job's inv_count     red here (1: the (4096, 1024) decode, the one case on that kernel); old: 14 red
  fold_compute: S and Cm swapped                      red here (19: fold, decode 10, backward 8); old: 13 red
  dec_bwd_sym_kernel without the transpose term       red here (8: every backward case, both entry points); old: 3 red
The older tolerance tests see all six -- the default-contrast ones too; what this file adds is the stage's name on the failure, the bit, and the
sizes past 10,000 pixels (profiles/r15/crossray_exact.txt).
"""
import numpy as np
import pytest
import torch

import _crossray_cases as C
from _crossray_cases import (APPLY_HW, BACKWARD, CHANSUM_HW, DECODE, GRAM_HW, GRAM_SEEDS, MATRIX_COUNTS, TWO_JOB, style_mean)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def first_difference(got, want):
    got, want = got.detach().cpu().reshape(-1), torch.as_tensor(want).reshape(-1)
    if torch.equal(got, want):
        return None
    bad = torch.nonzero((got != want) | torch.isnan(got)).reshape(-1)
    i = int(bad[0])
    return "%d of %d differ, first at %d: got %r, want %r" % (len(bad), want.numel(), i, float(got[i]), float(want[i]))


# ------------------------------------------------------------------------------------------------------------------ 1. the stages, bit for bit
@torch.no_grad()
@pytest.mark.parametrize("HW", CHANSUM_HW)
def test_chansum_bit_for_bit(HW):
    from crnerf_amd import ops
    c = C.chansum_case(HW)
    assert first_difference(ops.crossray_chansum(T(c["x"])), c["want"]) is None


@torch.no_grad()
@pytest.mark.parametrize("seed", GRAM_SEEDS)
@pytest.mark.parametrize("HW", GRAM_HW)
def test_gram_with_an_explicit_mean_bit_for_bit(HW, seed):
    from crnerf_amd import ops
    c = C.gram_case(HW, seed)
    got = ops.crossray_gram(T(c["x"]), T(c["mean"]), [T(t) for t in c["w"]])
    assert first_difference(got, c["want"]) is None


_zeros = {}


def _decoder_weights(snet, cnet):
    """22 tensors: the two conv chains of the cases; the fc layers and the fold, which phases 0 and 1 do not read, are zeros."""
    if not _zeros:
        _zeros.update(fc=torch.zeros(1024, 1024, device=DEV), b=torch.zeros(1024, device=DEV),
                      lin=[torch.zeros(n, device=DEV) for n in (32 * 64, 32, 64 * 32, 64, 3 * 64, 3)])
    return [T(t) for t in snet] + [_zeros["fc"], _zeros["b"]] + [T(t) for t in cnet] + [_zeros["fc"], _zeros["b"]] + _zeros["lin"]


@torch.no_grad()
@pytest.mark.parametrize("HW,HWs", TWO_JOB)
def test_two_job_gram_with_the_mean_from_sums_bit_for_bit(HW, HWs):
    """Phases 0 and 1 of the ray-sharded decode.  The content job's mean comes from `global` sums the test writes -- integer mean x a power-of-two
    count that is not the local pixel count, or zero sums with a ragged count --, the style job's from its own partial sums."""
    from crnerf_amd import ops
    ragged = (HW, HWs) == (1000, 4097)
    c, s = C.gram_case(HW, 2, "zero" if ragged else "int"), C.gram_case(HWs, 3, style_mean(HWs))
    count = 3000.0 if ragged else 65536.0
    assert count != HW and float(np.abs(c["mean"]).max()) * count < C.LIMIT
    w = _decoder_weights(s["w"], c["w"])
    x, sp = T(c["x"]), T(s["x"])
    ws = ops.crossray_workspace(x.device).view(torch.float32)
    ws[C.WS_STATS:C.WS_STATS + C.ST_SGRAM + 1024] = float("nan")
    xchg = torch.full((1088,), float("nan"), device=DEV)
    ops.crossray_decode_sharded(x, sp, w, 0, xchg, count)
    assert first_difference(xchg[:64], c["sums"]) is None
    xchg[:64] = T(c["mean"]) * count
    ops.crossray_decode_sharded(x, sp, w, 1, xchg, count)
    assert first_difference(xchg[64:], c["want"]) is None, "content Gram"
    st = ws[C.WS_STATS:]
    assert first_difference(st[C.ST_CMEAN:C.ST_CMEAN + 64], c["mean"]) is None, "content mean"
    assert first_difference(st[C.ST_SMEAN:C.ST_SMEAN + 64], s["mean"]) is None, "style mean"
    assert first_difference(st[C.ST_SGRAM:C.ST_SGRAM + 1024], s["want"]) is None, "style Gram"


@torch.no_grad()
@pytest.mark.parametrize("count", MATRIX_COUNTS)
def test_matrix_with_a_power_of_two_count_bit_for_bit(count):
    from crnerf_amd import ops
    c = C.matrix_case(count)
    assert first_difference(ops.crossray_matrix(T(c["g"]), count, T(c["w"]), T(c["b"])), c["want"]) is None


@torch.no_grad()
@pytest.mark.parametrize("count", [1000, 4097])
def test_matrix_with_a_ragged_count_inside_the_derived_bound(count):
    from crnerf_amd import ops
    c = C.matrix_case_dense(count)
    err = np.abs(ops.crossray_matrix(T(c["g"]), count, T(c["w"]), T(c["b"])).cpu().numpy().astype(np.float64) - c["want"])
    print("\ncount %d: worst error / bound %.3f" % (count, float((err / c["bound"]).max())))
    assert (err <= c["bound"]).all()


@torch.no_grad()
def test_fold_bit_for_bit():
    from crnerf_amd import ops
    c = C.fold_case()
    lin = [T(t) for t in c["lin"]]
    got = ops.crossray_fold(T(c["sM"]), T(c["cM"]), T(c["c_mean"]), T(c["s_mean"]), lin)
    assert first_difference(got, c["want"]) is None
    assert first_difference(got, c["swapped"]) is not None
    content = ops.crossray_fold(None, None, None, None, lin)                     # type == "content": the rgb conv alone
    assert first_difference(content, np.concatenate([c["lin"][4].reshape(-1), c["lin"][5]])) is None


@torch.no_grad()
@pytest.mark.parametrize("HW", APPLY_HW)
def test_apply_on_integer_pre_activations_into_a_strided_view(HW):
    from crnerf_amd import ops
    c = C.apply_case(HW)
    buf = torch.full((3, HW + 5), float("nan"), device=DEV)
    out = ops.crossray_apply(T(c["x"]), T(c["affine"]), out=buf[:, :HW])
    assert out.data_ptr() == buf.data_ptr() and torch.isfinite(buf[:, :HW]).all() and torch.isnan(buf[:, HW:]).all()
    got = buf[:, :HW].cpu()
    err = float((got.double() - torch.from_numpy(c["want"])).abs().max())
    print("\nHW %d: max |rgb - float64 sigmoid| %.2e" % (HW, err))
    assert err <= 1e-6
    # equal pre-activations, equal bits: one table entry per integer pre-activation
    pre = torch.from_numpy(c["pre"]).reshape(-1) + C.APPLY_RANGE
    bits = got.reshape(-1).view(torch.int32)
    table = torch.zeros(2 * C.APPLY_RANGE + 1, dtype=torch.int32)
    table[pre] = bits
    assert torch.equal(table[pre], bits)


# ------------------------------------------------------------------------------------------------------------------ 2. the whole decode, seeing
_decode = {}


def _decode_case(HW, HWs):
    if _decode.get("key") != (HW, HWs):
        case = C.decode_case(HW, HWs)
        ref, own, bar = C.decode_reference(case)
        _decode.clear()
        _decode.update(key=(HW, HWs), ref=torch.from_numpy(ref), own=own, bar=bar, x=T(case["content"]), s=T(case["style"]),
                       w=[T(t) for t in case["weights"]])
    return _decode


@torch.no_grad()
@pytest.mark.parametrize("HW,HWs", DECODE)
def test_decode_through_the_seeing_decoder(HW, HWs):
    from crnerf_amd import ops
    d = _decode_case(HW, HWs)
    err = float((ops.crossray_decode(d["x"], d["s"], d["w"]).cpu().double() - d["ref"]).abs().max())
    print("\n(%d, %d): max |rgb - float64| %.2e, bar %.1e (fp32 CPU oracle %.2e)" % (HW, HWs, err, d["bar"], d["own"]))
    assert err <= d["bar"]


@torch.no_grad()
@pytest.mark.parametrize("HW,HWs", DECODE)
def test_decode_composed_by_hand_from_the_five_stages(HW, HWs):
    from crnerf_amd import ops
    d = _decode_case(HW, HWs)
    x, s, w = d["x"], d["s"], d["w"]
    c_mean, s_mean = ops.crossray_chansum(x) / HW, ops.crossray_chansum(s) / HWs
    sM = ops.crossray_matrix(ops.crossray_gram(s, s_mean, w[0:6]), HWs, w[6], w[7])
    cM = ops.crossray_matrix(ops.crossray_gram(x, c_mean, w[8:14]), HW, w[14], w[15])
    rgb = ops.crossray_apply(x, ops.crossray_fold(sM, cM, c_mean, s_mean, w[16:22]))
    err = float((rgb.cpu().double() - d["ref"]).abs().max())
    print("\n(%d, %d) by hand: max |rgb - float64| %.2e, bar %.1e" % (HW, HWs, err, d["bar"]))
    assert err <= d["bar"]


# ------------------------------------------------------------------------------------------------------------------ 3. the backward, poisoned
_backward = {}


def _poison(shape):
    n = int(np.prod(shape))
    return torch.full((4 * n,), 0xff, dtype=torch.uint8, device=DEV).view(torch.float32).view(shape)


def _backward_case(HW, HWs):
    """Reference (float64 autograd), the three sharded phases on poisoned memory, the one-call backward: once per case."""
    if _backward.get("key") == (HW, HWs):
        return _backward
    from crnerf_amd import _lib, ops
    _backward.clear()
    torch.cuda.empty_cache()
    case = C.backward_case(HW, HWs)
    ref_dx, ref_ds, ref_g = C.backward_reference(case)
    x, s, d_rgb, w = T(case["content"]), T(case["style"]), T(case["d_rgb"]), [T(t) for t in case["weights"]]
    with torch.no_grad():
        xchg = torch.zeros(1088, device=DEV)
        for phase in (0, 1, 2):
            ops.crossray_decode_sharded(x, s, w, phase, xchg, float(HW))
        nbytes = _lib.load().crnerf_crossray_backward_workspace_bytes(HW, HWs)
        state = (torch.full((nbytes,), 0xff, dtype=torch.uint8, device=DEV), _poison((HW, 64)), _poison((HWs, 64)), [_poison(t.shape) for t in w])
        assert all(torch.isnan(t).all() for t in (state[1], state[2], state[3][0]))
        xb = torch.zeros(384, device=DEV)
        for phase in (0, 1, 2):
            ops.crossray_decode_backward_sharded(x, s, w, d_rgb, phase, xchg, float(HW), xb, state)
        one = ops.crossray_decode_backward(x, s, w, d_rgb)
        torch.cuda.synchronize()
    names = ["d_content", "d_style"] + C.weight_names()
    _backward.update(key=(HW, HWs), names=names, ref=[ref_dx, ref_ds] + [ref_g[k] for k in C.weight_names()],
                     sharded=[state[1].cpu(), state[2].cpu()] + [g.cpu() for g in state[3]], one=[one[0].cpu(), one[1].cpu()] + [g.cpu() for g in one[2]])
    return _backward


def _against_autograd(b, which):
    lines, bad = [], []
    for name, got, ref in zip(b["names"], b[which], b["ref"]):
        ref = torch.from_numpy(ref).reshape(got.shape)
        tol = C.backward_bar(ref.numpy())
        err = float((got.double() - ref).abs().max())
        lines.append("%s %.1e" % (name.replace("multi_net.", "").replace("decoder.feat_2_rgb_list.0", "rgb"), err / float(ref.abs().max())))
        if not err <= tol:
            bad.append("%s: %.3e > %.3e" % (name, err, tol))
    print("\n%s %s, worst error / max|ref| per tensor: %s" % (b["key"], which, ", ".join(lines)))
    return bad


@pytest.mark.parametrize("HW,HWs", BACKWARD)
def test_sharded_backward_on_poisoned_memory_vs_autograd_oracle(HW, HWs):
    b = _backward_case(HW, HWs)
    nan = [n for n, t in zip(b["names"], b["sharded"]) if not torch.isfinite(t).all()]
    assert not nan, "not finite: %s" % nan
    bad = _against_autograd(b, "sharded")
    assert not bad, bad


@pytest.mark.parametrize("HW,HWs", BACKWARD)
def test_one_call_backward_vs_autograd_oracle_and_the_sharded_phases(HW, HWs):
    b = _backward_case(HW, HWs)
    assert all(torch.isfinite(t).all() for t in b["one"])
    bad = _against_autograd(b, "one")
    # the bar of test_sharded_decoder_backward_adds_up_to_the_whole_grid (tests/test_gpu_train_aux.py): 3e-5 of the tensor's largest entry + 1e-8
    worst = 0.0
    for name, a, o in zip(b["names"], b["sharded"], b["one"]):
        err, top = float((a - o).abs().max()), float(o.abs().max())
        worst = max(worst, err / (top + 1e-30))
        if not err <= 3e-5 * top + 1e-8:
            bad.append("%s: the two entry points differ by %.3e, max %.3e" % (name, err, top))
    print("%s: the two entry points differ by at most %.1e of a tensor's largest entry" % (b["key"], worst))
    assert not bad, bad

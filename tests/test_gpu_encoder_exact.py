"""The appearance encoder's HIP kernels (csrc/encoder.hip, csrc/encoder_train.hip) held to the float64 reference BIT FOR BIT on inputs for which
every fp32 summation order is exact (tests/_encoder_cases.py: construction, certificate, reference; tests/test_encoder_exact_host.py: the
certificate and the power of these inputs, checked on the CPU).  torch.equal leaves no room for a wrong corner of the reflection adjoint, a wrong
tap on a border column, a wrong edge row of a GEMM tile or another tie rule in the max-pool backward -- none of which the tolerance tests of
test_gpu_parity.py / test_gpu_train_aux.py can see.  What this technique cannot see (LeakyReLU's negative branch inside the chain, averaging
windows of 3 rows) is covered at the end by a float64 comparison on general inputs, against the fp32 CPU oracle's own error.
"""
import os

import numpy as np
import pytest
import torch

import _encoder_cases as E

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_refs = {}


def _ref(name, bands=None):
    key = (name, None if bands is None else tuple(bands))
    if key not in _refs:
        _refs[key] = E.reference(E.get_case(name), bands=bands)
    return _refs[key]


def _dev(case):
    w = [torch.tensor(case["weights"][n], dtype=torch.float32, device=DEV) for n in E.NAMES]
    return w, torch.tensor(case["img"], dtype=torch.float32, device=DEV), torch.tensor(case["cot"], dtype=torch.float32, device=DEV)


def _same(got, want, what):
    """torch.equal against the float64 value rounded to fp32 (the certificate says it IS an fp32 number), with the first differing index in the message"""
    want32 = want.to(torch.float32)
    assert torch.equal(want32.double(), want.double()), what + ": the expected value is no fp32 number"
    got = got.detach().cpu()
    assert got.shape == want32.shape, (what, tuple(got.shape), tuple(want32.shape))
    if not torch.equal(got, want32):
        bad = (got != want32) | got.isnan()
        idx = tuple(int(v) for v in bad.nonzero()[0])
        raise AssertionError("%s: %d of %d elements differ, first at %s: got %r, want %r"
                             % (what, int(bad.sum()), bad.numel(), idx, float(got[idx]), float(want32[idx])))


def _module(case):
    from crnerf_amd.models.linearStyleTransfer import encoder_sameoutputsize
    enc = encoder_sameoutputsize(64).to(DEV)
    enc.load_state_dict({k: torch.tensor(v, dtype=torch.float32) for k, v in case["weights"].items()})
    return enc


@pytest.mark.parametrize("name", E.CASE_NAMES)
def test_forward_is_exact(name, monkeypatch):
    from crnerf_amd import ops
    case, ref = E.get_case(name), _ref(name)
    w, img, _ = _dev(case)
    with torch.no_grad():
        out = ops.encoder_forward(img, w)
        out_t, _, hw = ops.encoder_forward_train(img, w)
    assert hw == (case["H"], case["W"])
    _same(out, ref["out"], name + " encoder_forward")
    _same(out_t, ref["out"], name + " encoder_forward_train")
    assert torch.equal(out, out_t)
    # the drop-in module: the same bits, through the HIP entry point (not through its nn.Conv2d members)
    calls = []
    real = ops.encoder_forward
    monkeypatch.setattr(ops, "encoder_forward", lambda *a, **k: calls.append(1) or real(*a, **k))
    enc = _module(case)
    with torch.no_grad():
        grid = enc(img[None])
    assert calls == [1] and grid.shape == (1, 64, 32, 32)
    _same(E.pixel_major(grid), ref["out"], name + " encoder_sameoutputsize")


@pytest.mark.parametrize("name", E.CASE_NAMES)
def test_backward_is_exact(name):
    from crnerf_amd import ops
    case, ref = E.get_case(name), _ref(name)
    w, img, cot = _dev(case)
    with torch.no_grad():
        out, saved, hw = ops.encoder_forward_train(img, w)
        grads, d_img = ops.encoder_backward(w, saved, hw, out, cot)
        grads_only, none = ops.encoder_backward(w, saved, hw, out, cot, want_d_image=False)
    assert none is None
    for n, g, g2, want in zip(E.NAMES, grads, grads_only, ref["grads"]):
        _same(g, want, "%s d %s" % (name, n))
        _same(g2, want, "%s d %s (want_d_image=False)" % (name, n))
    _same(d_img, ref["d_img"], name + " d_image")
    # and through autograd on the drop-in module (autograd.EncoderFn)
    enc = _module(case)
    x = img[None].clone().requires_grad_()
    grid = enc(x)
    fn, chain = grid.grad_fn, []
    while fn is not None:
        chain.append(type(fn).__name__)
        fn = fn.next_functions[0][0] if fn.next_functions else None
    assert any("EncoderFn" in n for n in chain), chain
    (grid * E.cot_nchw(case, torch.float32).to(DEV)).sum().backward()
    _same(x.grad[0], ref["d_img"], name + " d_image (module)")
    assert [n for n, _ in enc.named_parameters()] == E.NAMES
    for (n, p), want in zip(enc.named_parameters(), ref["grads"]):
        _same(p.grad, want, "%s d %s (module)" % (name, n))


@pytest.mark.parametrize("name,ws", E.BAND_CASES)
def test_row_bands_are_exact(name, ws):
    """Every band's owned rows of the style grid ARE the reference's rows; its gradients are the reference's for the cotangent restricted to those
    rows (exact term by term, so the float64 sum over the bands is the whole image's gradient, bit for bit)."""
    from crnerf_amd import ops
    from crnerf_amd.parallel import encoder_band_plan
    case = E.get_case(name)
    H, W = case["H"], case["W"]
    plans = [encoder_band_plan(H, W, ws, rank) for rank in range(ws)]
    ref = _ref(name, bands=[(p[3], p[4]) for p in plans])
    w, img, cot = _dev(case)
    sum_g = [torch.zeros(t.shape, dtype=torch.float64) for t in ref["grads"]]
    sum_d = torch.zeros(3, H, W, dtype=torch.float64)
    with torch.no_grad():
        for rank, ((_, row0, rows, o0, o1, _), rb) in enumerate(zip(plans, ref["bands"])):
            tag = "%s band %d/%d" % (name, rank, ws)
            own, saved, hw = ops.encoder_forward_train_band(img[:, row0:row0 + rows].contiguous(), H, row0, o0, o1, w)
            _same(own, ref["out"][o0 * 32:o1 * 32], tag + " output rows")
            grads, d_rows = ops.encoder_backward_band(w, saved, hw, H, row0, o0, o1, own, cot[o0 * 32:o1 * 32].contiguous())
            for n, g, want, acc in zip(E.NAMES, grads, rb["grads"], sum_g):
                _same(g, want, "%s d %s" % (tag, n))
                acc += g.cpu().double()
            _same(d_rows, rb["d_img"][:, row0:row0 + rows], tag + " d_image rows")
            sum_d[:, row0:row0 + rows] += d_rows.cpu().double()
    for n, acc, want in zip(E.NAMES, sum_g, ref["grads"]):
        assert torch.equal(acc, want), n
    assert torch.equal(sum_d, ref["d_img"])


@pytest.mark.parametrize("name", E.CASE_NAMES)
def test_negative_branch_of_the_last_activation(name):
    """conv7's bias moved down until about half of its outputs are negative: out = float32(0.2) * float32(v) there, ONE rounding of an exact v --
    the activation epilogue of enc_gemm_nt_kernel<true> (everywhere else in these cases LeakyReLU is the identity)."""
    from crnerf_amd import ops
    case, want = E.sign_case(E.get_case(name))
    w, img, _ = _dev(case)
    with torch.no_grad():
        out = ops.encoder_forward(img, w)
        out_t = ops.encoder_forward_train(img, w)[0]
    _same(out, torch.from_numpy(want), name + " encoder_forward")
    _same(out_t, torch.from_numpy(want), name + " encoder_forward_train")


PARITY_K = 2.0      # e_hip <= K * e_ref: the next power of two above the worst ratio measured on the MI355X (1.01 at 176x8, profiles/r9/encoder_parity.txt)


@pytest.mark.parametrize("H,W", E.PARITY_SHAPES)
def test_forward_vs_float64_on_general_inputs(H, W):
    """Signed dense weights (synth.encoder_state), ragged shapes, and (176, 8) whose quarter-resolution map of 44 rows is averaged over windows of
    3 rows: ops.encoder_forward and the fp32 CPU oracle, each against the float64 oracle, element by element.  The bar is the suite's own
    (2e-5 max|ref| + 1e-6, test_appearance_encoder_golden) or PARITY_K times the fp32 CPU oracle's own error, whichever is larger.
    CRNERF_ENCODER_PARITY_OUT=<file>: the figures are appended there (profiles/r9/encoder_parity.txt)."""
    import crnerf_amd.synth as synth
    from crnerf_amd import ops
    from oracle import cpu_ref as O
    st = synth.encoder_state(51, 2.0)
    img = torch.rand(1, 3, H, W, generator=torch.Generator().manual_seed(H * 1000 + W))
    ref = E.pixel_major(O.encoder_forward({k: torch.from_numpy(v).double() for k, v in st.items()}, img.double()))
    cpu = E.pixel_major(O.encoder_forward(O.to_torch(st), img)).double()
    with torch.no_grad():
        hip = ops.encoder_forward(img.to(DEV), [torch.from_numpy(st[n]).to(DEV) for n in E.NAMES]).cpu().double()
    e_ref, e_hip, scale = float((cpu - ref).abs().max()), float((hip - ref).abs().max()), float(ref.abs().max())
    floor = 2e-5 * scale + 1e-6
    line = "%3dx%-3d max|ref| %.3e  e_ref %.3e  e_hip %.3e  ratio %.2f  floor %.3e" % (H, W, scale, e_ref, e_hip, e_hip / max(e_ref, 1e-30), floor)
    print("\n" + line)
    if os.environ.get("CRNERF_ENCODER_PARITY_OUT"):
        with open(os.environ["CRNERF_ENCODER_PARITY_OUT"], "a") as f:
            f.write(line + "\n")
    assert (ref < 0).any() and (ref > 0).any()                     # both branches of the last activation
    assert e_hip <= max(floor, PARITY_K * e_ref), line
    assert np.isfinite(e_hip)

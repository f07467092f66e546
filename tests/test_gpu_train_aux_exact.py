"""The three kernels of csrc/train_aux.hip that run on every training step -- the Adam step, the fused loss with its gradient, the grid-sample
batcher -- held BIT FOR BIT to the NumPy restatements of tests/_train_aux_cases.py (which tests/test_train_aux_exact_host.py ties to float64,
torch.optim.Adam and the reference's recorded outputs), on the paths the older tests never reach: more tensors than one launch carries, the
scalar branch of the Adam kernel, absent gradients across blocks and at a launch's edge, the padding of the flat buffers, two parameter groups,
a resumed state; the loss at its 256-block cap and in a second sweep, with a non-ray tensor deciding the grid, every optional-input
combination, strided targets, a workspace reused after a larger call; batches whose size is no multiple of the block, both roundings, a row
offset, wider ray rows."""
import copy

import numpy as np
import pytest
import torch

import _train_aux_cases as C
from crnerf_amd import _lib, ops, optim
from crnerf_amd.datasets.phototourism_mask_grid_sample import GridSampleBatcher

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HYPER = dict(lr=5e-4, betas=(0.9, 0.999), eps=1e-8)
WD = 2.0 ** -7          # a power of two: weight_decay * p is exact, the fused multiply-add is one fp32 addition (no double rounding in the restatement)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _same(got, want):
    return torch.equal(got.detach().cpu().reshape(-1), torch.from_numpy(np.ascontiguousarray(want)).reshape(-1))


# ---------------------------------------------------------------- Adam
def _grad(g, sliced):
    """The gradient as a fresh allocation (16-byte aligned: the kernel's vector branch), or as the contiguous slice buf[1:1+n] (its scalar branch)."""
    if g is None:
        return None
    if not sliced:
        return _dev(g)
    buf = torch.zeros(g.size + 1, device=DEV)
    t = buf[1:1 + g.size]
    t.copy_(torch.from_numpy(g))
    assert t.is_contiguous() and t.data_ptr() % 16 == 4
    return t


def _assert_state(opt, ps, ref, what):
    for k, p in enumerate(ps):
        st = opt.state[p]
        for name, got, want in (("p", p, ref[0][k]), ("exp_avg", st["exp_avg"], ref[1][k]), ("exp_avg_sq", st["exp_avg_sq"], ref[2][k])):
            assert _same(got, want), (what, "tensor %d" % k, name, float(np.abs(got.detach().cpu().numpy().reshape(-1).astype(np.float64) - want).max()))


def _run(sizes, grads, wd, sliced=False, seed=1):
    """Ten FlatAdam steps, every one compared with adam_step32 on p, exp_avg and exp_avg_sq of every tensor.  Returns the optimiser and its parameters."""
    p0 = C.adam_params(sizes, seed)
    ps = [torch.nn.Parameter(_dev(a)) for a in p0]
    opt = optim.FlatAdam(ps, weight_decay=wd, **HYPER)
    ref = [[a.copy() for a in p0], [np.zeros_like(a) for a in p0], [np.zeros_like(a) for a in p0]]
    for t, row in enumerate(grads, 1):
        for k, g in enumerate(row):
            ps[k].grad = _grad(g, sliced)
            if g is not None:
                ref[0][k], ref[1][k], ref[2][k] = C.adam_step32(ref[0][k], ref[1][k], ref[2][k], g, wd=wd, t=t, **HYPER)
        opt.step()
        _assert_state(opt, ps, ref, "step %d" % t)
    return opt, ps


def _padding_is_zero(fg):
    keep = torch.ones(fg.flat.numel(), dtype=torch.bool)
    for p, off in zip(fg.params, fg.offsets):
        keep[off:off + p.numel()] = False
    assert int(keep.sum()) > 0
    return all(not bool(buf.cpu()[keep].any()) for buf in (fg.flat, fg.exp_avg, fg.exp_avg_sq))


ZERO = {2: 0, 7: 5, 10: 0}          # exact zeros from step 1 (v = 0, denom = eps, quotient 0), also across three blocks; exact zeros from step 6


@pytest.mark.parametrize("wd", [0.0, WD])
def test_adam_step_bit_for_bit_and_padding_stays_zero(wd):
    """Every size around the vector path's tail and the 4096-element block split, gradients over eight decades and exact zeros: parameters and
    both moments equal the restatement bit for bit after each of ten steps; the padding between the tensors is still zero in all three buffers."""
    assert int(_lib.load().crnerf_adam_max_tensors()) == C.ADAM_MAX_TENSORS
    opt, ps = _run(C.ADAM_SIZES, C.adam_grads(C.ADAM_SIZES, 2, zero=ZERO), wd)
    assert _padding_is_zero(opt._groups[0])
    if wd == 0:
        assert torch.equal(ps[2].detach().cpu(), torch.from_numpy(C.adam_params(C.ADAM_SIZES, 1)[2]))     # zero gradients from the start: nothing moves


@pytest.mark.parametrize("wd", [0.0, WD])
def test_adam_step_scalar_branch_equals_the_vector_branch(wd):
    """Every gradient a contiguous slice buf[1:1+n] (4 bytes past a 16-byte boundary): the kernel's scalar branch.  Same restatement, and the
    same bits as the aligned run."""
    grads = C.adam_grads(C.ADAM_SIZES, 3, zero=ZERO)
    a, pa = _run(C.ADAM_SIZES, grads, wd, sliced=False)
    b, pb = _run(C.ADAM_SIZES, grads, wd, sliced=True)
    for x, y in zip(pa, pb):
        assert torch.equal(x.detach(), y.detach()) and torch.equal(a.state[x]["exp_avg"], b.state[y]["exp_avg"])
        assert torch.equal(a.state[x]["exp_avg_sq"], b.state[y]["exp_avg_sq"])
    assert _padding_is_zero(b._groups[0])


@pytest.mark.parametrize("n_tensors", [449, 897])
def test_adam_step_over_more_tensors_than_one_launch_carries(n_tensors):
    """449 and 897 tensors of 1 to 70 elements: two and three launches per step, the tensor index restarting in each while the flat offsets stay
    global.  Tensors 0, 447, 448 (and 896) carry gradients of their own pattern; tensor 200 has 8193 elements (three blocks) and never a gradient;
    tensors 447 and 448 -- either side of the first launch's edge -- miss one step each.  The three flat buffers, padding included, equal
    the restatement bit for bit after every step."""
    rng = np.random.default_rng(n_tensors)
    sizes = [int(n) for n in rng.integers(1, 71, n_tensors)]
    sizes[200] = 8193
    p0 = C.adam_params(sizes, 7)
    ps = [torch.nn.Parameter(_dev(a)) for a in p0]
    opt = optim.FlatAdam(ps, weight_decay=WD, **HYPER)
    fg = opt._groups[0]
    assert len(fg.chunks) == -(-n_tensors // C.ADAM_MAX_TENSORS) and fg.chunks[1].blocks[0, 0].item() == 0 and fg.chunks[1].blocks[0, 1].item() == fg.offsets[448]
    goff = np.concatenate([[0], np.cumsum([-(-n // 4) * 4 for n in sizes])])          # gradients: 16-byte aligned views of ONE upload per step
    flat = [np.zeros(fg.flat.numel(), np.float32) for _ in range(3)]
    for a, off in zip(p0, fg.offsets):
        flat[0][off:off + a.size] = a
    marked = [k for k in (0, 447, 448, 896) if k < n_tensors]
    grads = C.adam_grads(sizes, 8)
    for t, row in enumerate(grads, 1):
        for k in marked:
            row[k] = ((k + 1) * 1e-3 * (1 + np.arange(sizes[k])) * (-1) ** t).astype(np.float32)
        absent = {200} | ({447} if t == 3 else set()) | ({448} if t == 5 else set())
        host = np.zeros(goff[-1], np.float32)
        for k, g in enumerate(row):
            host[goff[k]:goff[k] + g.size] = g
        dev = _dev(host)
        for k, p in enumerate(ps):
            p.grad = None if k in absent else dev[goff[k]:goff[k] + sizes[k]]
            if k not in absent:
                sl = slice(fg.offsets[k], fg.offsets[k] + sizes[k])
                flat[0][sl], flat[1][sl], flat[2][sl] = C.adam_step32(flat[0][sl], flat[1][sl], flat[2][sl], row[k], wd=WD, t=t, **HYPER)
        opt.step()
        for name, got, want in (("p", fg.flat, flat[0]), ("exp_avg", fg.exp_avg, flat[1]), ("exp_avg_sq", fg.exp_avg_sq, flat[2])):
            bad = np.nonzero(got.cpu().numpy() != want)[0]
            assert bad.size == 0, (t, name, "first differing flat element %d of %d" % (bad[0], bad.size))
    assert _padding_is_zero(fg)
    sl = slice(fg.offsets[200], fg.offsets[200] + 8193)
    assert np.array_equal(flat[0][sl], p0[200]) and not flat[1][sl].any() and not flat[2][sl].any()       # (and so the device's, compared above)
    for k in marked:                                                                                       # the state views are those slices
        sl = slice(fg.offsets[k], fg.offsets[k] + sizes[k])
        assert _same(ps[k], flat[0][sl]) and _same(opt.state[ps[k]]["exp_avg"], flat[1][sl]) and _same(opt.state[ps[k]]["exp_avg_sq"], flat[2][sl])


def test_adam_step_two_parameter_groups_each_with_its_own_constants():
    sizes = [(5, 65, 4097), (3, 64, 8193)]
    hyper = [dict(lr=1e-3, betas=(0.8, 0.99), wd=0.0), dict(lr=5e-4, betas=(0.9, 0.999), wd=WD)]
    p0 = [C.adam_params(s, 20 + i) for i, s in enumerate(sizes)]
    ps = [[torch.nn.Parameter(_dev(a)) for a in grp] for grp in p0]
    opt = optim.FlatAdam([dict(params=ps[i], lr=h["lr"], betas=h["betas"], weight_decay=h["wd"]) for i, h in enumerate(hyper)], eps=1e-8)
    ref = [[[a.copy() for a in grp], [np.zeros_like(a) for a in grp], [np.zeros_like(a) for a in grp]] for grp in p0]
    grads = [C.adam_grads(s, 30 + i) for i, s in enumerate(sizes)]
    for t in range(1, 11):
        for i, h in enumerate(hyper):
            for k, g in enumerate(grads[i][t - 1]):
                ps[i][k].grad = _dev(g)
                ref[i][0][k], ref[i][1][k], ref[i][2][k] = C.adam_step32(ref[i][0][k], ref[i][1][k], ref[i][2][k], g, lr=h["lr"], betas=h["betas"],
                                                                         eps=1e-8, wd=h["wd"], t=t)
        opt.step()
        for i in range(2):
            _assert_state(opt, ps[i], ref[i], "group %d step %d" % (i, t))


def test_adam_step_resumes_a_torch_layout_state_at_step_100000():
    sizes = (5, 4097, 8193)
    p0 = C.adam_params(sizes, 40)
    rng = np.random.default_rng(41)
    m0 = [(0.1 * rng.standard_normal(n)).astype(np.float32) for n in sizes]
    v0 = [(1e-2 * rng.standard_normal(n) ** 2 + 1e-12).astype(np.float32) for n in sizes]
    ps = [torch.nn.Parameter(_dev(a)) for a in p0]
    opt = optim.FlatAdam(ps, weight_decay=WD, **HYPER)
    sd = copy.deepcopy(opt.state_dict())
    sd["state"] = {k: {"step": torch.tensor(100000.0), "exp_avg": torch.from_numpy(m0[k]), "exp_avg_sq": torch.from_numpy(v0[k])} for k in range(len(sizes))}
    opt.load_state_dict(sd)
    _assert_state(opt, ps, (p0, m0, v0), "loaded")
    g = C.adam_grads(sizes, 42, steps=1)[0]
    for k, p in enumerate(ps):
        p.grad = _dev(g[k])
    opt.step()
    ref = [C.adam_step32(p0[k], m0[k], v0[k], g[k], wd=WD, t=100001, **HYPER) for k in range(len(sizes))]
    _assert_state(opt, ps, list(zip(*ref)), "step 100001")
    assert float(opt.state_dict()["state"][0]["step"]) == 100001


@pytest.mark.parametrize("wd,decades,floor", [(1e-2, (-6, 2), 1e-15), (1e-2, (-30, -6), 1e-30), (0.0, (-30, -6), 1e-30)])
def test_adam_step_general_weight_decay_and_tiny_gradients_within_the_float64_bars(wd, decades, floor):
    """Where the restatement is no safe bitwise reference -- a general weight_decay (the float64 emulation of fmaf can round twice), gradients
    down to 1e-30 (g^2 is subnormal or 0 in fp32) -- every step is held to adam_step64 FROM THE DEVICE'S OWN STATE before it, inside the counted
    bars, plus one subnormal step 2^-149 on exp_avg_sq."""
    sizes = (5, 65, 4097, 8193)
    ps = [torch.nn.Parameter(_dev(a)) for a in C.adam_params(sizes, 50)]
    opt = optim.FlatAdam(ps, weight_decay=wd, **HYPER)
    read = lambda: [(p.detach().cpu().numpy().copy(), opt.state[p]["exp_avg"].cpu().numpy().copy(), opt.state[p]["exp_avg_sq"].cpu().numpy().copy()) for p in ps]  # noqa: E731
    worst = np.zeros(3)
    for t, row in enumerate(C.adam_grads(sizes, 51, floor=floor, decades=decades), 1):
        before = read()
        for p, g in zip(ps, row):
            p.grad = _dev(g)
        opt.step()
        for k, (b, a, g) in enumerate(zip(before, read(), row)):
            p64, m64, v64, bars = C.adam_step64(b[0], b[1], b[2], g, wd=wd, t=t, **HYPER)
            for j, (got, want, bar) in enumerate(((a[0], p64, bars[0]), (a[1], m64, bars[1]), (a[2], v64, bars[2] + 2.0 ** -149))):
                err = np.abs(got.astype(np.float64) - want)
                assert (err <= bar).all(), (t, k, "pmv"[j], float((err / bar).max()))
                worst[j] = max(worst[j], float((err / bar).max()))
    print("device vs float64 one-step bars, worst error / bar (p, m, v): %.3f %.3f %.3f" % tuple(worst))


# ---------------------------------------------------------------- loss
_GRAD_NAME = {"rgb_coarse": "rgb_coarse", "rgb_fine": "rgb_fine", "mask": "mask", "a": "a_embedded", "a_rec": "a_embedded_random_rec", "c_wo": "content_wo",
              "c_with": "content_with"}


def _loss_device(case, mse_a=False, upstream=C.LOSS_UPSTREAM, view=None):
    """crnerf_loss_f32 and crnerf_loss_backward_f32 through ops.loss_args; view: re-lays the device tensors out (strided inputs)."""
    t = {k: _dev(v) for k, v in case.items() if v is not None}
    if view is not None:
        t = view(t)
    args, keep = ops.loss_args(t["rgb_coarse"], t["targets"], rgb_fine=t.get("rgb_fine"), mask=t.get("mask"), a_embedded=t.get("a"),
                               a_embedded_random=t.get("a_rand"), a_embedded_random_rec=t.get("a_rec"), content_wo=t.get("c_wo"), content_with=t.get("c_with"),
                               mse_on_appearance=mse_a, **C.LOSS_CFG)
    val = ops.loss_forward(args)
    want = {_GRAD_NAME[k]: tuple(case[k].shape) for k in _GRAD_NAME if case.get(k) is not None}
    if "mask" in want:                       # what the allocator hands loss_backward next is not zeros: d_mask must be WRITTEN, also where it is 0
        junk = torch.full(want["mask"], float("nan"), device=DEV)
        del junk
    grads = ops.loss_backward(args, _dev(upstream), want)
    return val.cpu().numpy(), {k: grads[_GRAD_NAME[k]].cpu().numpy() for k in _GRAD_NAME if _GRAD_NAME[k] in grads}


def _assert_loss(case, mse_a=False, view=None, upstream=C.LOSS_UPSTREAM):
    val, grads = _loss_device(case, mse_a, upstream, view)
    want = C.loss_forward32(case, mse_a=mse_a)
    assert np.array_equal(val, want), [(k, float(a), float(b)) for k, a, b in zip(C.LOSS_KEYS, val, want) if a != b]
    ref = C.loss_backward32(case, upstream, mse_a=mse_a)
    assert set(grads) == set(ref)
    for k in ref:
        bad = np.nonzero(grads[k].reshape(-1) != ref[k].reshape(-1))[0]
        assert bad.size == 0, (k, "%d elements differ, first %d: %r vs %r" % (bad.size, bad[0], grads[k].reshape(-1)[bad[0]], ref[k].reshape(-1)[bad[0]]))
    return val, grads


@pytest.mark.parametrize("mse_a", [False, True])
@pytest.mark.parametrize("R", C.LOSS_ROWS)
def test_loss_bit_for_bit_up_to_the_block_cap_and_a_second_sweep(R, mse_a):
    """One block, block edges, the 256-block cap (262144 rows), one row past it and 300001 rows (a second sweep of 37857 threads); mask values
    exactly 0 / 0.5 / 1 and a_rand == a_rec planted at the first and last rows; arbitrary upstream weights with a zero and a negative."""
    case = C.loss_case(R, seed=R)
    _, grads = _assert_loss(case, mse_a)
    if not mse_a:
        assert grads["a_rec"][0] == 0 and grads["a_rec"][-1] == 0


@pytest.mark.parametrize("kw", [dict(n_c=2049), dict(n_a=300001)], ids=["n_c2049", "n_a300001"])
def test_loss_grid_decided_by_a_non_ray_tensor(kw):
    _assert_loss(C.loss_case(5, seed=60, **kw))
    _assert_loss(C.loss_case(5, seed=61, **kw), mse_a=True)


@pytest.mark.parametrize("kw", [dict(fine=False), dict(mask=False), dict(rec=False), dict(a=False), dict(a=False, content=False, mask=False, fine=False)],
                         ids=["mask_without_fine", "fine_without_mask", "a_without_a_rec", "content_pair_alone", "coarse_alone"])
def test_loss_every_optional_input_combination(kw):
    case = C.loss_case(1025, seed=62, **kw)
    val, grads = _assert_loss(case)
    if kw == dict(fine=False):
        assert not grads["mask"].any() and not np.isnan(grads["mask"]).any() and val[4] == 0 and val[5] == 0 and val[6] == 0


def test_loss_strided_inputs_equal_the_contiguous_run():
    case = C.loss_case(1025, seed=63)
    base = _assert_loss(case)

    def planar(names):
        def view(t):
            for k in names:
                t[k] = t[k].t().contiguous().t()
                assert not t[k].is_contiguous()
            return t
        return view

    def wide(t):
        buf = torch.rand(t["targets"].shape[0], 8, device=DEV)
        buf[:, :3] = t["targets"]
        t["targets"] = buf[:, :3]
        assert t["targets"].stride() == (8, 1)
        return t
    for view in (planar(["targets"]), wide, planar(["rgb_coarse", "rgb_fine"]), planar(["targets", "rgb_coarse", "rgb_fine"])):
        got = _assert_loss(case, view=view)
        assert np.array_equal(got[0], base[0]) and all(np.array_equal(got[1][k], base[1][k]) for k in base[1])


def test_loss_workspace_reused_after_a_larger_call():
    small, large = C.loss_case(257, seed=64), C.loss_case(300001, seed=65)
    fresh = _assert_loss(small)                 # 1 block
    _assert_loss(large)                         # 256 blocks of partial sums in the same workspace
    again = _assert_loss(small)
    assert np.array_equal(fresh[0], again[0])


# ---------------------------------------------------------------- grid-sample batcher
@pytest.mark.parametrize("rounding", ["floor", "round"])
@pytest.mark.parametrize("side", C.BATCH_SIDES)
def test_grid_sample_batch_bit_for_bit_where_the_block_guard_fires(side, rounding):
    """side^2 = 1, 9, 289, 1089 samples (no multiple of 256): the first and the last image of a four-image buffer (a non-zero row offset), ray
    rows of 9 and of 11 floats, a draw with scale 1 and zero offsets (the lattice's largest w_lin / h_lin) and a general one."""
    for width in (9, 11):
        rays, rgbs, off = C.batch_buffers(seed=side, ray_width=width)
        b = GridSampleBatcher(_dev(rays), _dev(rgbs), np.array(C.BATCH_WH))
        assert b.all_rays.shape[1] == width and [int(o) for o in b._offsets] == [int(o) for o in off]
        for img in (0, len(C.BATCH_WH) - 1):
            w, h = C.BATCH_WH[img]
            lw, lh = b._lin(w, side), b._lin(h, side)
            for scale, h_off, w_off in ((1.0, 0.0, 0.0), (0.6, 0.3 * (1 - 1 / h), 0.25 * (1 - 1 / w))):
                want = C.grid_batch32(rays, rgbs, int(off[img]), w, h, side, lw.cpu().numpy(), lh.cpu().numpy(), scale, h_off, w_off, rounding)
                assert want["inside"]                                           # decided on the host, before anything is launched
                got = ops.grid_sample_batch(b.all_rays, b.all_rgbs, int(off[img]), w, h, side, lw, lh, scale, h_off, w_off, rounding=rounding)
                for k in ("rays", "ts", "rgbs", "rgb_idx", "uv_sample"):
                    a = got[k].cpu().numpy()
                    assert a.dtype == want[k].dtype and np.array_equal(a, want[k]), (k, width, img, scale)

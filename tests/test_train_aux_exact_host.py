"""The NumPy restatements of csrc/train_aux.hip's three per-step kernels (tests/_train_aux_cases.py) held to float64, to torch.optim.Adam and to
the reference's recorded outputs -- on the host.  tests/test_gpu_train_aux_exact.py then holds the kernels to the restatements bit for bit."""
import math

import numpy as np
import pytest
import torch

import _train_aux_cases as C

f32, f64, U = np.float32, np.float64, C.U
HYPER = dict(lr=5e-4, betas=(0.9, 0.999), eps=1e-8)


@pytest.mark.parametrize("wd", [0.0, 2.0 ** -7, 1e-2])
def test_adam_step32_lies_within_the_counted_bars_of_float64(wd):
    """Ten steps of the fp32 restatement; at every step the float64 evaluation of the SAME step from the same fp32 state is within the counted
    bars (adam_step64's docstring), for gradients over eight decades, exact zeros from step 6 on one tensor, and a general weight decay."""
    sizes = C.ADAM_SIZES
    p = np.concatenate(C.adam_params(sizes, 1))
    m, v = np.zeros_like(p), np.zeros_like(p)
    worst = np.zeros(3)
    for t, row in enumerate(C.adam_grads(sizes, 2, zero={7: 5}), 1):
        g = np.concatenate(row)
        p64, m64, v64, bars = C.adam_step64(p, m, v, g, wd=wd, t=t, **HYPER)
        p, m, v = C.adam_step32(p, m, v, g, wd=wd, t=t, **HYPER)
        for k, (got, want, bar) in enumerate(((p, p64, bars[0]), (m, m64, bars[1]), (v, v64, bars[2]))):
            err = np.abs(got.astype(f64) - want)
            assert (err <= bar).all(), (t, "pmv"[k], float((err / np.maximum(bar, 1e-300)).max()))
            worst[k] = max(worst[k], float((err[bar > 0] / bar[bar > 0]).max()))
    print("adam_step32 vs float64, worst error / bar (p, m, v): %.3f %.3f %.3f" % tuple(worst))


@pytest.mark.parametrize("wd", [0.0, 1e-2])
def test_adam_step64_is_torch_adam_on_float64(wd):
    """Ties the formula to torch: ten steps of adam_step64 on the Python-double constants against torch.optim.Adam on float64 CPU tensors."""
    sizes = (1, 5, 65, 4097)
    ps = [a.astype(f64) for a in C.adam_params(sizes, 3)]
    ms, vs = [np.zeros_like(a) for a in ps], [np.zeros_like(a) for a in ps]
    tp = [torch.nn.Parameter(torch.from_numpy(a.copy())) for a in ps]
    opt = torch.optim.Adam(tp, weight_decay=wd, **HYPER)
    for t, row in enumerate(C.adam_grads(sizes, 4), 1):
        for k, g in enumerate(row):
            tp[k].grad = torch.from_numpy(g.astype(f64))
            ps[k], ms[k], vs[k], _ = C.adam_step64(ps[k], ms[k], vs[k], g, wd=wd, t=t, scalars="f64", **HYPER)
        opt.step()
    for k in range(len(sizes)):
        st = opt.state[tp[k]]
        assert float(st["step"]) == 10
        for got, want in ((ps[k], tp[k].detach().numpy()), (ms[k], st["exp_avg"].numpy()), (vs[k], st["exp_avg_sq"].numpy())):
            assert (np.abs(got - want) <= 1e-12 * np.abs(want)).all(), (k, float((np.abs(got - want) / np.abs(want)).max()))


def test_one_minus_beta_formed_in_fp32_falls_outside_the_second_moment_bar():
    """The defect this pin found, as arithmetic: 1.0f - (float)0.999 = 0.00099998713 where torch hands its kernels (float)(1 - 0.999) =
    0.00100000005, 1.29e-5 relative apart (beta1: 2.4e-7).  A second moment built with the former lies about 36 bars outside 6u v' wherever the
    gradient term carries v' (first step, |g| >= 1e-3) -- so the bar separates the two, and the moment assertions fail on the fp32 form."""
    b1, b2 = HYPER["betas"]
    bad2, good2 = f32(1.0) - f32(b2), f32(1.0 - b2)
    assert abs(float(bad2) / float(good2) - 1) > 1.28e-5 and abs(float(good2) / (1.0 - b2) - 1) < U
    assert abs(float(f32(1.0) - f32(b1)) / (1.0 - b1) - 1) > 2.3e-7 and abs(float(f32(1.0 - b1)) / (1.0 - b1) - 1) < U
    rng = np.random.default_rng(5)
    g = rng.standard_normal(100000).astype(f32)
    g = g[np.abs(g) >= 1e-3]
    p = rng.standard_normal(g.size).astype(f32)
    z = np.zeros_like(p)
    _, _, v64, bars = C.adam_step64(p, z, z, g, wd=0.0, t=1, **HYPER)
    _, _, v_good = C.adam_step32(p, z, z, g, wd=0.0, t=1, **HYPER)
    _, _, v_bad = C.adam_step32(p, z, z, g, wd=0.0, t=1, omb2=bad2, **HYPER)
    assert (np.abs(v_good - v64) <= bars[2]).all()
    assert (np.abs(v_bad - v64) > 30 * bars[2]).all()
    rel = np.abs(v_bad - v64) / v64
    assert 1.27e-5 < float(np.median(rel)) < 1.31e-5


class HP:
    maskrs_max, maskrs_min, maskrs_k, maskrd = 5e-2, 6e-3, 1e-3, 1e-3
    weightKL, weightRecA, weightcontent = 1e-5, 1e-3, 1e-4


@pytest.mark.parametrize("tag", ["full", "mse_a", "nomask", "coarse_only"])
def test_loss_restatement_reproduces_the_reference_outputs(golden, tag):
    """loss_forward32 / loss_backward32 on golden g10_loss at the bars tests/test_gpu_train_aux.py holds the kernel to."""
    g = golden("g10_loss")
    case = C.golden_loss_case(g, tag)
    cfg = dict(coef=1.0, weight_kl=HP.weightKL, weight_rec_a=HP.weightRecA, weight_content=HP.weightcontent,
               mask_size_weight=float(g[tag + "__ann"]), mask_digit_weight=HP.maskrd)
    keys = list(g[tag + "__keys"])
    val = C.loss_forward32(case, cfg, mse_a=tag == "mse_a")
    for k, name in enumerate(C.LOSS_KEYS):
        if name in keys:
            want = float(g[tag + "__loss_" + name])
            assert abs(float(val[k]) - want) <= 2e-6 * abs(want) + 1e-12, (name, float(val[k]), want)
        else:
            assert val[k] == 0, name
    upstream = np.array([1.0 if name in keys else 0.0 for name in C.LOSS_KEYS], f32)          # backward of the plain sum of the dict's values
    grads = C.loss_backward32(case, upstream, cfg, mse_a=tag == "mse_a")
    for name, key in (("rgb_coarse", "d_rgb_coarse"), ("rgb_fine", "d_rgb_fine"), ("mask", "d_mask"), ("a", "d_a"), ("a_rec", "d_a_rand_rec"),
                      ("c_wo", "d_c_wo"), ("c_with", "d_c_with")):
        want = g[tag + "__" + key]
        if name in grads:
            np.testing.assert_allclose(grads[name].reshape(want.shape), want, rtol=2e-5, atol=2e-10, err_msg=name)
        else:
            assert not want.any(), name


HOST_LOSS_CASES = [dict(R=1), dict(R=257), dict(R=4096), dict(R=300001), dict(R=5, n_c=2049), dict(R=5, n_a=300001), dict(R=1025, fine=False),
                   dict(R=1025, mask=False), dict(R=1023, rec=False), dict(R=255, a=False)]


@pytest.mark.parametrize("mse_a", [False, True])
@pytest.mark.parametrize("kw", HOST_LOSS_CASES, ids=lambda kw: "-".join("%s%s" % kv for kv in kw.items()))
def test_loss_restatement_lies_within_the_counted_bars_of_float64(kw, mse_a):
    """Values within (ceil(n/nthr) + 12) u sum|addends| scale and gradients within 8u of their addends (loss64's docstring has the counts)."""
    case = C.loss_case(seed=11, **kw)
    val64, g64, bars, mag = C.loss64(case, C.LOSS_UPSTREAM, mse_a=mse_a)
    val = C.loss_forward32(case, mse_a=mse_a)
    for k, name in enumerate(C.LOSS_KEYS):
        assert abs(float(val[k]) - val64[k]) <= bars[k], (name, float(val[k]), val64[k], bars[k])
    grads = C.loss_backward32(case, C.LOSS_UPSTREAM, mse_a=mse_a)
    assert set(grads) == set(g64)
    for name in grads:
        err = np.abs(grads[name].astype(f64) - g64[name])
        assert (err <= 8 * U * mag[name]).all(), (name, float((err / np.maximum(mag[name], 1e-300)).max() / U))
    if case["a_rec"] is not None and not mse_a:
        assert grads["a_rec"][0] == 0 and grads["a_rec"][-1] == 0               # a_rand == a_rec: the L1 gradient is exactly 0
    if case["mask"] is not None and case["rgb_fine"] is None:
        assert not grads["mask"].any()


@pytest.mark.parametrize("tag", ["a", "b", "c"])
def test_batcher_restatement_reproduces_the_reference_batches(golden, tag):
    """grid_batch32 on golden g11_batcher, exactly; the host-side draws are GridSampleBatcher.draw's."""
    from crnerf_amd.datasets.phototourism_mask_grid_sample import GridSampleBatcher
    g = golden("g11_batcher")
    v = lambda k: g[tag + "__" + k]  # noqa: E731
    b = GridSampleBatcher(torch.from_numpy(g["all_rays"]), torch.from_numpy(g["all_rgbs"]), g["wh"], batch_size=int(v("batch")),
                          scale_anneal=float(v("anneal")), min_scale=float(v("min_scale")))
    b.iterations = int(v("iterations"))
    torch.manual_seed(int(v("torch_seed")))
    ts, img_w, img_h, cur, scale, h_off, w_off = b.draw(int(v("idx")), current_epoch=int(v("epoch")))
    assert cur == float(v("min_scale_cur")) and [img_w, img_h] == list(v("img_wh"))
    side = int(math.sqrt(int(v("batch"))))
    got = C.grid_batch32(g["all_rays"], g["all_rgbs"], int(b._offsets[ts]), img_w, img_h, side, b._lin(img_w, side).numpy(), b._lin(img_h, side).numpy(),
                         scale, h_off, w_off)
    assert got["inside"]
    for k in ("rays", "ts", "rgbs", "rgb_idx", "uv_sample"):
        assert got[k].dtype == v(k).dtype and np.array_equal(got[k], v(k)), k

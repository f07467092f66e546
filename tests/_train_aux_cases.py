"""NumPy restatements of the three per-step kernels of csrc/train_aux.hip -- the Adam step, the fused loss with its gradient, the grid-sample
batcher -- and the seeded cases that the host and GPU tests share (tests/test_train_aux_exact_host.py, tests/test_gpu_train_aux_exact.py).

The library is built with -ffp-contract=off, so every `*`, `+`, `-`, `/` and sqrtf of those kernels is ONE correctly rounded fp32 operation, which
is what a NumPy float32 array operation is; the only fused operation is adam_one's explicit fmaf(weight_decay, p, g).  The `...32` functions
restate the kernels operation for operation (and, for the loss sums, in the kernel's own fixed summation order), so the device is held to them
bit for bit; the `...64` functions evaluate the same formulas in float64 and carry the rounding COUNTS that tie the restatements to them.

NumPy only: no torch, no device, no reference import."""
import math

import numpy as np

f32, f64 = np.float32, np.float64
U = 2.0 ** -24                       # unit roundoff of fp32

# ---------------------------------------------------------------- Adam
ADAM_SIZES = (1, 3, 4, 5, 63, 64, 65, 4095, 4096, 4097, 8193, 12289)      # the vector path's tail (n % 4) and the 4096-element block split
ADAM_MAX_TENSORS = 448               # csrc/kernels.h; the GPU tests assert crnerf_adam_max_tensors() == this


def adam_scalars(lr, betas, eps, wd, t):
    """The six fp32 constants of AdamHyper that the update reads, formed as FlatAdam.step and the entry form them: step_size and
    bias_correction2_sqrt in Python double, then rounded; 1 - beta in double, then rounded (NOT 1.0f - (float)beta)."""
    b1, b2 = betas
    return dict(step_size=f32(lr / (1.0 - b1 ** t)), bc2=f32(math.sqrt(1.0 - b2 ** t)), beta2=f32(b2), omb1=f32(1.0 - b1), omb2=f32(1.0 - b2),
                eps=f32(eps), wd=f32(wd))


def fma32(a, b, c):
    """fmaf as the float64 product-sum rounded to fp32 (the product of two fp32 numbers is exact in float64)."""
    return (np.asarray(a, f64) * np.asarray(b, f64) + np.asarray(c, f64)).astype(f32)


def adam_step32(p, m, v, g, lr, betas, eps, wd, t, omb2=None):
    """adam_one, operation for operation in fp32.  omb2: override the second-moment weight (the host test plants the parent commit's
    1.0f - (float)beta2 there).  Returns (p', m', v')."""
    s = adam_scalars(lr, betas, eps, wd, t)
    w2 = s["omb2"] if omb2 is None else f32(omb2)
    p, m, v, g = (np.asarray(a, f32) for a in (p, m, v, g))
    if s["wd"] != 0:
        g = fma32(s["wd"], p, g)
    m2 = m + (g - m) * s["omb1"]
    v2 = s["beta2"] * v + (w2 * g) * g
    denom = np.sqrt(v2) / s["bc2"] + s["eps"]
    p2 = p - s["step_size"] * (m2 / denom)
    assert p2.dtype == m2.dtype == v2.dtype == f32
    return p2, m2, v2


def adam_step64(p, m, v, g, lr, betas, eps, wd, t, scalars="f32"):
    """The same formula in float64.  scalars="f32": on the kernel's fp32-rounded constants (a one-step comparison from identical fp32 state);
    scalars="f64": on the Python doubles (what torch.optim.Adam computes on float64 tensors).  Returns (p', m', v', bars) with bars =
    (dp, dm, dv), the distance an fp32 evaluation of ONE step from the same state may lie away.  Rounding is counted, not measured; with
    u = 2^-24, g' = g + wd p, den = sqrt(v')/bc2 + eps, upd = step_size m'/den:
      |dm'| <= 4u (|m| + |g'|)   4 roundings -- the fma, g' - m, the product with 1 - beta1, the sum -- each of a quantity <= |m| + |g'|
      |dv'| <= 6u v'             g' carries u, so g'^2 carries 2u; (1-beta2) g', its product with g', beta2 v and the sum add 4; every
                                 addend is non-negative, so relative errors do not amplify
      |dp'| <= u (|p| + |upd|)   the final subtraction
               + 9u |upd|        sqrt, / bc2, + eps, m'/den, the product with step_size = 5; v' carries 6u, 3u through the square root; 1 for
                                 the second-order terms
               + step_size 4u (|m| + |g'|) / den      dm' carried through the quotient."""
    b1, b2 = betas
    if scalars == "f32":
        s = {k: f64(x) for k, x in adam_scalars(lr, betas, eps, wd, t).items()}
    else:
        s = dict(step_size=lr / (1.0 - b1 ** t), bc2=math.sqrt(1.0 - b2 ** t), beta2=b2, omb1=1.0 - b1, omb2=1.0 - b2, eps=eps, wd=wd)
    p, m, v, g = (np.asarray(a, f64) for a in (p, m, v, g))
    g = g + s["wd"] * p
    m2 = m + (g - m) * s["omb1"]
    v2 = s["beta2"] * v + s["omb2"] * g * g
    den = np.sqrt(v2) / s["bc2"] + s["eps"]
    upd = s["step_size"] * (m2 / den)
    dm = 4 * U * (np.abs(m) + np.abs(g))
    dv = 6 * U * v2
    dp = U * (np.abs(p) + np.abs(upd)) + 9 * U * np.abs(upd) + s["step_size"] * dm / den
    return p - upd, m2, v2, (dp, dm, dv)


def adam_params(sizes, seed):
    rng = np.random.default_rng(seed)
    return [rng.standard_normal(n).astype(f32) for n in sizes]


def adam_grads(sizes, seed, steps=10, zero=None, floor=1e-15, decades=(-6, 2)):
    """steps x tensors gradients: randn * 10^U{-6..1} per tensor and step.  zero: {tensor index: first step (0-based) from which the gradient
    is exactly 0}.  |g| >= floor or exactly 0, so that no intermediate of the update is subnormal (g^2 (1 - beta2) >= 1e-33)."""
    rng = np.random.default_rng(seed)
    out = []
    for step in range(steps):
        row = []
        for k, n in enumerate(sizes):
            g = (rng.standard_normal(n) * 10.0 ** float(rng.integers(*decades))).astype(f32)
            if floor:
                small = (g != 0) & (np.abs(g) < floor)
                g[small] = np.copysign(f32(floor), g[small])
            if zero and k in zero and step >= zero[k]:
                g = np.zeros(n, f32)
            row.append(g)
        out.append(row)
    return out


# ---------------------------------------------------------------- loss
LOSS_KEYS = ("kl_a", "rec_a_random", "c_l", "content_constraint", "r_ms", "r_md", "f_l")
LOSS_BLOCKS, LOSS_THREADS = 256, 256
LOSS_CFG = dict(coef=1.0, weight_kl=1e-5, weight_rec_a=1e-3, weight_content=1e-4, mask_size_weight=0.0145562871, mask_digit_weight=1e-3)


def loss_blocks(c):
    n = max(c["R"], c["n_a"], c["n_rec"], c["n_c"])
    return int(min(max((n + 1023) // 1024, 1), LOSS_BLOCKS))


def _sizes(case):
    """R and the three element counts as to_loss_args sets them (a count is 0 when its tensor is absent)."""
    return dict(R=case["rgb_coarse"].shape[0], n_a=case["a"].size if case.get("a") is not None else 0,
                n_rec=case["a_rec"].size if case.get("a_rec") is not None else 0, n_c=case["c_wo"].size if case.get("c_wo") is not None else 0)


def loss_scales(case, cfg, dtype=f32):
    """to_loss_args: the struct's fields are fp32, the expression is double, the scale is rounded to fp32 (dtype=f64: left unrounded)."""
    z = _sizes(case)
    c, R = f64(f32(cfg["coef"])), f64(z["R"])
    w = lambda k: f64(f32(cfg[k]))  # noqa: E731
    reg = case.get("mask") is not None and case.get("rgb_fine") is not None
    s = [c * w("weight_kl") / f64(z["n_a"]) if z["n_a"] else 0.0, c * w("weight_rec_a") / f64(z["n_rec"]) if z["n_rec"] else 0.0, c * 0.5 / (3.0 * R),
         c * w("weight_content") / f64(z["n_c"]) if z["n_c"] else 0.0, c * w("mask_size_weight") / R if reg else 0.0,
         c * w("mask_digit_weight") / R if reg else 0.0, c * 0.5 / (3.0 * R) if case.get("rgb_fine") is not None else 0.0]
    return np.array(s, f64).astype(dtype)


def _terms(case, mse_a, dt):
    """Per-element addends of the seven sums, in the kernel's association, in dtype dt (None: the term has no addends)."""
    one, half, c002 = dt(1.0), dt(0.5), dt(f32(0.02)) if dt is f32 else dt(0.02)
    R = case["rgb_coarse"].shape[0]
    tg, rc = case["targets"].astype(dt), case["rgb_coarse"].astype(dt)
    m = case["mask"].reshape(-1).astype(dt) if case.get("mask") is not None else np.zeros(R, dt)

    def sq3(x):
        d = x - tg
        return ((dt(0.0) + d[:, 0] * d[:, 0]) + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    ec = sq3(rc)
    ef = sq3(case["rgb_fine"].astype(dt)) if case.get("rgb_fine") is not None else np.zeros(R, dt)
    t = [None] * 7
    t[2], t[6] = (one - m) * ec, (one - m) * ef
    if case.get("mask") is not None:
        t[4] = m * m
        t[5] = one / ((m - half) * (m - half) + c002)
    if case.get("a") is not None:
        a = case["a"].reshape(-1).astype(dt)
        t[0] = a * a
    if case.get("a_rec") is not None:
        d = case["a_rand"].reshape(-1).astype(dt) - case["a_rec"].reshape(-1).astype(dt)
        t[1] = d * d if mse_a else np.abs(d)
    if case.get("c_wo") is not None:
        d = case["c_wo"].reshape(-1).astype(dt) - case["c_with"].reshape(-1).astype(dt)
        t[3] = d * d
    return t, ef


def _block_sums32(term, nblk):
    """loss_partial_kernel's sum of one term: thread tid adds rows tid, tid + nthr, ... in fp32; six xor-butterfly levels d = 32 ... 1 inside
    each 64-lane wave (lane 0's value is kept); the four wave sums left to right.  Returns partial[nblk] (fp32)."""
    nthr = nblk * LOSS_THREADS
    sweeps = -(-term.size // nthr)
    pad = np.zeros(sweeps * nthr, f32)
    pad[:term.size] = term
    acc = np.zeros(nthr, f32)
    for row in pad.reshape(sweeps, nthr):          # an absent row adds nothing in the kernel; + 0.0f changes no value
        acc = acc + row
    v = acc.reshape(nblk, 4, 64)
    lane = np.arange(64)
    for d in (32, 16, 8, 4, 2, 1):
        v = v + v[:, :, lane ^ d]
    w = v[:, :, 0]
    return ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]


def loss_forward32(case, cfg=LOSS_CFG, mse_a=False):
    """crnerf_loss_f32: losses[7] (fp32), bit for bit -- the summation order of loss_partial_kernel / loss_final_kernel is fixed."""
    nblk = loss_blocks(_sizes(case))
    sc = loss_scales(case, cfg)
    terms, _ = _terms(case, mse_a, f32)
    out = np.zeros(7, f32)
    for k in range(7):
        total = 0.0
        if terms[k] is not None:
            for b in _block_sums32(terms[k], nblk):          # double, ascending block order
                total += float(b)
        out[k] = f32(total * float(sc[k]))
    return out


def loss_backward32(case, upstream, cfg=LOSS_CFG, mse_a=False):
    """crnerf_loss_backward_f32, element for element with C's left-to-right association.  Returns every gradient the inputs allow:
    rgb_coarse, rgb_fine, mask, a, a_rec, c_wo, c_with (flat where the input is flat)."""
    sc = loss_scales(case, cfg)
    u = np.asarray(upstream, f32) * sc
    two, one, half = f32(2.0), f32(1.0), f32(0.5)
    R = case["rgb_coarse"].shape[0]
    tg = case["targets"].astype(f32)
    has_m, has_f = case.get("mask") is not None, case.get("rgb_fine") is not None
    m = case["mask"].reshape(-1) if has_m else np.zeros(R, f32)
    out = {"rgb_coarse": (u[2] * two * (one - m))[:, None] * (case["rgb_coarse"] - tg)}
    ef = np.zeros(R, f32)
    if has_f:
        df = case["rgb_fine"] - tg
        ef = ((f32(0.0) + df[:, 0] * df[:, 0]) + df[:, 1] * df[:, 1]) + df[:, 2] * df[:, 2]
        out["rgb_fine"] = (u[6] * two * (one - m))[:, None] * df
    if has_m:
        e = m - half
        q = e * e + f32(0.02)
        out["mask"] = ((u[4] * two * m - (u[5] * two * e) / (q * q)) - u[6] * ef) if has_f else np.zeros(R, f32)
    if case.get("a") is not None:
        out["a"] = u[0] * two * case["a"].reshape(-1)
    if case.get("a_rec") is not None:
        d = case["a_rand"].reshape(-1) - case["a_rec"].reshape(-1)
        out["a_rec"] = (-u[1] * two) * d if mse_a else -u[1] * np.sign(d)
    if case.get("c_wo") is not None:
        d = u[3] * two * (case["c_wo"].reshape(-1) - case["c_with"].reshape(-1))
        out["c_wo"], out["c_with"] = d, -d
    assert all(v.dtype == f32 for v in out.values())
    return out


def loss64(case, upstream, cfg=LOSS_CFG, mse_a=False):
    """The reference's formulas (losses.py:49-96, as tests/test_gpu_train_aux.py::test_loss_upstream_weights_and_color_loss writes them) in
    float64 on the ABI's inputs (the struct's weights are fp32 fields).  Returns (losses[7], grads, value_bars[7], grad_addends):
    value_bars[k] = (ceil(n_k / nthr) + 12) u * sum|addends| * scale_k.  The count: ceil(n/nthr) - 1 additions in a thread's chain, 6 butterfly
    levels and 3 wave additions (the double sum over blocks is below 2^-29 u), the scale's rounding to fp32, the final rounding = ceil(n/nthr) +
    10; the remaining 2 are for forming an addend.  An addend costs 1 (a^2) to 7 roundings ((1 - m) sum_c (rgb - t)^2: 3 per square, 2 additions,
    1 - m, the product), but those are independent per element and each is relative to ITS addend, so across a sum they enter as a mean, not
    as a worst case; where a sum has few addends the chain and tree additions add zeros and are exact, which leaves the 7 + 3 <= 12.
    grad_addends[name] = sum of |addends| of that gradient (d_mask has three of either sign); gradients are held to 8u of it: at most two
    roundings in u[k] = upstream * scale, one per further product or difference."""
    z = _sizes(case)
    sc = loss_scales(case, cfg, f64)
    terms, ef = _terms(case, mse_a, f64)
    nthr = loss_blocks(z) * LOSS_THREADS
    val, bars = np.zeros(7), np.zeros(7)
    for k in range(7):
        if terms[k] is not None:
            val[k] = terms[k].sum() * sc[k]
            bars[k] = (-(-terms[k].size // nthr) + 12) * U * np.abs(terms[k]).sum() * sc[k]
    u = np.asarray(upstream, f32).astype(f64) * sc
    R = z["R"]
    tg = case["targets"].astype(f64)
    has_m, has_f = case.get("mask") is not None, case.get("rgb_fine") is not None
    m = case["mask"].reshape(-1).astype(f64) if has_m else np.zeros(R)
    g = {"rgb_coarse": (u[2] * 2 * (1 - m))[:, None] * (case["rgb_coarse"] - tg)}
    if has_f:
        g["rgb_fine"] = (u[6] * 2 * (1 - m))[:, None] * (case["rgb_fine"] - tg)
    mag = {}
    if has_m:
        q = (m - 0.5) ** 2 + 0.02
        parts = (u[4] * 2 * m, -u[5] * 2 * (m - 0.5) / (q * q), -u[6] * ef) if has_f else (np.zeros(R),) * 3
        g["mask"] = parts[0] + parts[1] + parts[2]
        mag["mask"] = np.abs(parts[0]) + np.abs(parts[1]) + np.abs(parts[2])
    if z["n_a"]:
        g["a"] = u[0] * 2 * case["a"].reshape(-1).astype(f64)
    if z["n_rec"]:
        d = case["a_rand"].reshape(-1).astype(f64) - case["a_rec"].reshape(-1)
        g["a_rec"] = -u[1] * 2 * d if mse_a else -u[1] * np.sign(d)
    if z["n_c"]:
        d = u[3] * 2 * (case["c_wo"].reshape(-1).astype(f64) - case["c_with"].reshape(-1))
        g["c_wo"], g["c_with"] = d, -d
    for k in g:
        mag.setdefault(k, np.abs(g[k]))
    return val, g, bars, mag


LOSS_ROWS = (1, 255, 256, 257, 1023, 1025, 4096, 262144, 262145, 300001)      # one block ... the 256-block cap ... a second sweep of every thread
LOSS_UPSTREAM = np.array([1.0, 2.0, 3.0, 0.0, -2.0, 7.0, 0.5], f32)           # arbitrary upstream weights with a zero and a negative


def loss_case(R, seed, fine=True, mask=True, a=True, rec=True, content=True, n_a=4096, n_c=1024):
    """A seeded loss input.  Planted at the first and last rows: mask exactly 0 / 0.5 / 1, a_rand == a_rec (an L1 gradient of exactly 0)."""
    rng = np.random.default_rng(seed)
    u = lambda *s: rng.random(s, dtype=f32)  # noqa: E731
    c = {"rgb_coarse": u(R, 3), "targets": u(R, 3), "rgb_fine": u(R, 3) if fine else None, "mask": None, "a": None, "a_rand": None, "a_rec": None,
         "c_wo": None, "c_with": None}
    if mask:
        m = u(R, 1)
        for i, x in ((0, 0.0), (1, 0.5), (R - 2, 0.5), (R - 1, 1.0)):
            if 0 <= i < R:
                m[i] = x
        c["mask"] = m
    if a:
        c["a"] = rng.standard_normal(n_a).astype(f32)
        if rec:
            c["a_rand"], c["a_rec"] = rng.standard_normal(n_a).astype(f32), rng.standard_normal(n_a).astype(f32)
            c["a_rec"][[0, -1]] = c["a_rand"][[0, -1]]
    if content:
        c["c_wo"], c["c_with"] = rng.standard_normal(n_c).astype(f32), rng.standard_normal(n_c).astype(f32)
    return c


def golden_loss_case(g, tag):
    """The inputs of golden g10_loss as a case, with the optional inputs the reference's call had for that tag."""
    v = lambda k: g[tag + "__" + k]  # noqa: E731
    keys = list(g[tag + "__keys"])
    return {"rgb_coarse": v("rgb_coarse"), "targets": v("targets"), "rgb_fine": v("rgb_fine") if "f_l" in keys else None,
            "mask": v("mask") if tag in ("full", "mse_a") else None, "a": v("a"), "a_rand": v("a_rand"), "a_rec": v("a_rand_rec"), "c_wo": v("c_wo"),
            "c_with": v("c_with")}


# ---------------------------------------------------------------- grid-sample batcher
BATCH_WH = ((29, 31), (51, 80), (37, 23), (41, 19))          # (w, h) of the four images of the buffer
BATCH_SIDES = (1, 3, 17, 33)                                 # side^2 = 1, 9, 289, 1089: none a multiple of the 256-thread block


def batch_buffers(seed=0, ray_width=9):
    """all_rays[N, ray_width] (column 8 = the image's id, further columns unread), all_rgbs[N,3], row offsets of the images."""
    rng = np.random.default_rng(seed)
    sizes = [w * h for w, h in BATCH_WH]
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    rays = rng.standard_normal((int(off[-1]), ray_width)).astype(f32)
    rays[:, 8] = np.repeat(np.arange(len(sizes)) + 3, sizes)
    return rays, rng.random((int(off[-1]), 3), dtype=f32), off


def grid_batch32(all_rays, all_rgbs, row_offset, img_w, img_h, side, w_lin, h_lin, scale, h_offset, w_offset, rounding="floor"):
    """grid_batch_kernel<ROUND>: all arithmetic in fp32 with separate multiplications and additions; sample n = j * side + i reads w_lin[i] and
    h_lin[j].  Returns the five outputs and "inside": whether every sampled pixel lies in the image (to be checked BEFORE anything is launched)."""
    n = np.arange(side * side)
    i, j = n % side, n // side
    w_lin, h_lin = np.asarray(w_lin, f32), np.asarray(h_lin, f32)
    w_sb = w_lin[i] * f32(scale) + f32(w_offset)
    h_sb = h_lin[j] * f32(scale) + f32(h_offset)
    wf, hf = w_sb * f32(img_w), h_sb * f32(img_h)
    rnd = np.rint if rounding == "round" else np.floor
    w, h = rnd(wf), rnd(hf)
    ptf = w + h * f32(img_w)
    assert ptf.dtype == f32
    pt = ptf.astype(np.int64)
    inside = bool((w >= 0).all() and (w < img_w).all() and (h >= 0).all() and (h < img_h).all() and (pt + row_offset < all_rays.shape[0]).all())
    row = np.clip(pt + row_offset, 0, all_rays.shape[0] - 1)
    return {"rays": all_rays[row, :8], "ts": all_rays[row, 8].astype(np.int64), "rgbs": all_rgbs[row], "rgb_idx": pt,
            "uv_sample": np.stack([h_sb, w_sb], 1), "inside": inside}

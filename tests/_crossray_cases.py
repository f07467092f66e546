"""Cases, certificates and references for the bit-exact tests of the cross-ray decoder (csrc/crossray.hip): tests/test_crossray_exact_host.py (CPU)
and tests/test_gpu_crossray_exact.py (device).  NumPy int64 / float64 (and float64 torch autograd for the backward); nothing here touches a device.

The method is the one of the encoder and MLP-gradient pins: inputs on which EVERY fp32 summation order gives the same bits, so that the kernels'
sums -- whatever their tiling, their tree or their launch split -- are compared with torch.equal against an int64 evaluation.  A sum of fp32
numbers that are all integer multiples of one quantum is exact in any order when sum |terms| < 2^24 quanta: every partial sum is then an
integer below 2^24 quanta, which fp32 holds.  Each constructor below builds its case, then CERTIFIES it in integer arithmetic and refuses
(AssertionError) a case that fails.

  channel sums   x = small signed integers * 2^-4; sum_px |x| < 2^24 quanta per channel.
  Gram           the chain 64 -> 128 -> 64 -> 32 with lrelu(v) = v > 0 ? v : 0.2f * v after the first two convs.  0.2f * v in fp32 equals v / 5
                 exactly when v is a multiple of 5 (0.2f = 0.2 (1 + 2^-26); the product rounds back to the integer -- asserted for every value
                 used).  x - mean in {0, +-25}, integer weights (one or two nonzeros per row), b1 in multiples of 25, b2 in multiples of 5, b3
                 integer: first pre-activations are multiples of 25, second ones multiples of 5, every activation an integer, and
                 sum_px |h3_i h3_j| < 2^24.  Biases are negative and rare: biases of both signs overflow the bound at 32,801 pixels.
  matrix         integer Gram sums, sparse integer fc weights, integer bias, power-of-two count (quantum 1 / count).
  fold           small integers everywhere; every partial sum of U = Wrgb Wunzip, U S, (U S) Cm, A and v below 2^24.
"""
import numpy as np

LIMIT = 1 << 24
WS_STATS = 2 * 256 * 64 + 2 * 256 * 1024          # csrc/crossray.hip: WS_STATS (floats); the statistics block the backward reads
ST_CMEAN, ST_SMEAN, ST_CGRAM, ST_SGRAM = 0, 64, 128, 128 + 1024


# the sizes of tests/test_gpu_crossray_exact.py, each the smallest that crosses a switch of csrc/crossray.hip (the host test certifies the same)
CHANSUM_HW = (1, 63, 64, 65, 4096, 4097, 16384, 16385, 16449, 32801, 131073)
GRAM_HW = (1, 31, 32, 33, 127, 129, 4095, 4096, 4097, 4128, 32768, 32769, 32801)
GRAM_SEEDS = (0, 1)
TWO_JOB = ((33, 1024), (4097, 1024), (1000, 4097), (4097, 8193), (32801, 33))
MATRIX_COUNTS = (1024, 4096, 65536)
APPLY_HW = (1, 63, 65, 131072, 131073, 131137)
DECODE = ((4096, 1024), (4097, 1024), (1000, 4097), (4097, 4097), (32801, 1024))
BACKWARD = ((4097, 1024), (8225, 1024), (32801, 1024), (33, 4097))


def style_mean(HWs):
    """Power-of-two style grids carry nonzero integer means; ragged ones sum to zero in every channel (mean 0 whatever 1 / HWs rounds to)."""
    return "int" if HWs & (HWs - 1) == 0 else "zero"


def bits(v):
    """log2 of a certificate's left-hand side: 24 is the limit."""
    return float(np.log2(max(float(v), 1.0)))


# ------------------------------------------------------------------------------------------------------------------ channel sums
def chansum_case(HW, seed=0):
    rng = np.random.default_rng(1000 + seed + HW)
    q = rng.integers(-15, 16, size=(HW, 64), dtype=np.int64)
    worst = int(np.abs(q).sum(0).max())
    assert worst < LIMIT, "channel sums: %d quanta" % worst
    return {"HW": HW, "x": (q * 2.0 ** -4).astype(np.float32), "want": (q.sum(0) * 2.0 ** -4).astype(np.float32), "bits": bits(worst)}


# ------------------------------------------------------------------------------------------------------------------ Gram
def sparse_int(rng, rows, cols, nnz, vals):
    w = np.zeros((rows, cols), np.int64)
    for r in range(rows):
        w[r, rng.choice(cols, nnz[r], replace=False)] = rng.choice(vals, nnz[r])
    return w


def cnn_weights(seed, small=False):
    """[w1, b1, w2, b2, w3, b3] as int64.  Seed parity picks the weight family: two +-1 per row, or one / two nonzeros per row -- of +-1, +-2 on
    grids of a few hundred pixels (small), of +-1 beyond (each layer of +-2 costs two bits of the Gram's 24)."""
    rng = np.random.default_rng(2000 + seed)
    if seed % 2 == 0:
        nnz, vals = (lambda n: np.full(n, 2)), [-1, 1]
    else:
        nnz, vals = (lambda n: rng.integers(1, 3, n)), ([-2, -1, 1, 2] if small else [-1, 1])
    w1, w2, w3 = sparse_int(rng, 128, 64, nnz(128), vals), sparse_int(rng, 64, 128, nnz(64), vals), sparse_int(rng, 32, 64, nnz(32), vals)
    b1 = -25 * (rng.random(128) < 0.1).astype(np.int64)
    b2 = -5 * (rng.random(64) < 0.1).astype(np.int64)
    b3 = (rng.random(32) < 0.1) * rng.choice([-1, 1], 32)
    return [w1, b1, w2, b2, w3, b3.astype(np.int64)]


def imm(a, b):
    """Integer matrix product through the float64 BLAS (exact: every entry and partial sum is an integer far below 2^53), back in int64."""
    assert max(np.abs(a).max(initial=0), np.abs(b).max(initial=0)) < 1 << 20 and a.shape[1] <= 1024
    return (a.astype(np.float64) @ b.astype(np.float64)).astype(np.int64)


def lrelu_int(p):
    """lrelu02 on multiples of 5, in integers -- with the proof that fp32 does the same on every value that occurs."""
    assert (p % 5 == 0).all(), "pre-activation that is no multiple of 5"
    neg = np.unique(p[p < 0])
    assert (np.float32(0.2) * neg.astype(np.float32) == (neg // 5).astype(np.float32)).all(), "0.2f * v != v / 5 in fp32"
    return np.where(p > 0, p, p // 5)


def chain_int(d, w):
    """d = x - mean [HW,64] int64 -> (p1, p2, h3): the two pre-activations and the chain's output."""
    w1, b1, w2, b2, w3, b3 = w
    p1 = imm(d, w1.T) + b1
    assert (p1 % 25 == 0).all(), "first pre-activation that is no multiple of 25"
    p2 = imm(lrelu_int(p1), w2.T) + b2
    return p1, p2, imm(lrelu_int(p2), w3.T) + b3


def density(HW, seed):
    """P(x - mean != 0): as dense as the Gram's 24 bits allow; the family of seed parity 1 has fewer weights per row and takes half as many again."""
    return (0.25 if HW < 256 else (0.125 if HW <= 8300 else 0.0625)) * (1.5 if seed % 2 and HW > 256 else 1.0)


def centred(HW, rng, zero_sum, seed=0):
    """x - mean in {0, +-25}.  zero_sum: as many +25 as -25 in every channel, so the channel sums of x - (integer mean) vanish."""
    p = density(HW, seed)
    if not zero_sum or HW < 2:
        return 25 * rng.choice([-1, 1], size=(HW, 64)) * (rng.random((HW, 64)) < p)
    d = np.zeros((HW, 64), np.int64)
    n = max(1, int(round(p * HW / 2)))
    for c in range(64):
        idx = rng.choice(HW, 2 * n, replace=False)
        d[idx[:n], c], d[idx[n:], c] = 25, -25
    return d


def gram_case(HW, seed, mean="int", zero_sum=True):
    """mean: "int" (integers in -3..3, not all zero) or "zero".  Returns x, the mean, the weights (fp32 and int64), the reference and the margins."""
    rng = np.random.default_rng(3000 + 17 * seed + HW)
    d = centred(HW, rng, zero_sum, seed)
    m = rng.integers(-3, 4, size=64) if mean == "int" else np.zeros(64, np.int64)
    if mean == "int":
        m[0], m[1] = 3, -2
    w = cnn_weights(seed, small=HW <= 256)
    p1, p2, h3 = chain_int(d, w)
    worst = int((np.abs(h3).T @ np.abs(h3)).max())
    assert worst < LIMIT, "Gram: sum |h3_i h3_j| = %d" % worst
    assert (np.abs(h3).sum(1) > 0).all(), "a pixel with h3 = 0 would not be missed"
    frac = {}
    if HW >= 127:                                   # (a handful of pixels cannot hold a fraction)
        for name, p in (("1", p1), ("2", p2)):
            frac[name] = (float((p > 0).mean()), float((p < 0).mean()))
            assert min(frac[name]) >= 0.05, "layer %s takes one lrelu branch for %.3f of its activations only" % (name, min(frac[name]))
    x = d + m
    csum = int(np.abs(x).sum(0).max())
    assert csum < LIMIT
    return {"HW": HW, "x": x.astype(np.float32), "mean": m.astype(np.float32), "w_int": w, "w": [t.astype(np.float32) for t in w],
            "d": d, "sums": x.sum(0).astype(np.float32), "want": (h3.T @ h3).reshape(-1).astype(np.float32), "bits": bits(worst), "branches": frac,
            "h3": h3}


# ------------------------------------------------------------------------------------------------------------------ matrix
def ref_matrix(gram_sum, count, fc_w, fc_b):
    return np.asarray(fc_w, np.float64) @ (np.asarray(gram_sum, np.float64) / float(count)) + np.asarray(fc_b, np.float64)


def matrix_case(count, seed=0):
    """Exact: integer Gram sums, four integer weights per row, integer bias, power-of-two count."""
    assert count & (count - 1) == 0
    rng = np.random.default_rng(4000 + seed + count)
    g = rng.integers(-(1 << 20), (1 << 20) + 1, size=1024, dtype=np.int64)
    w = sparse_int(rng, 1024, 1024, np.full(1024, 4), [-2, -1, 1, 2])
    b = rng.integers(-3, 4, size=1024, dtype=np.int64)
    worst = int((np.abs(w) @ np.abs(g) + np.abs(b) * count).max())        # in quanta of 1 / count
    assert worst < LIMIT, "matrix: %d quanta" % worst
    want = ref_matrix(g, count, w, b)
    assert (want.astype(np.float32).astype(np.float64) == want).all()
    return {"count": count, "g": g.astype(np.float32), "w": w.astype(np.float32), "b": b.astype(np.float32), "want": want.astype(np.float32),
            "bits": bits(worst)}


def matrix_case_dense(count, seed=0):
    """Any count: dense random-sign inputs against float64, with the order-independent bound
    (1024 + 2) 2^-24 (sum_k |w_k g_k| / count + |b|): the rounding of 1 / count, of g / count, and of at most 1024 additions per row."""
    rng = np.random.default_rng(5000 + seed + count)
    g = (rng.normal(size=1024) * 0.25 * count).astype(np.float32)
    w = rng.uniform(-1 / 32, 1 / 32, size=(1024, 1024)).astype(np.float32)
    b = rng.uniform(-1 / 32, 1 / 32, size=1024).astype(np.float32)
    bound = 1026 * 2.0 ** -24 * (np.abs(w.astype(np.float64)) @ np.abs(g.astype(np.float64)) / count + np.abs(b.astype(np.float64)))
    return {"count": count, "g": g, "w": w, "b": b, "want": ref_matrix(g, count, w, b), "bound": bound}


# ------------------------------------------------------------------------------------------------------------------ fold
def ref_fold(sM, cM, c_mean, s_mean, lin):
    """A [3,64] and v [3] of rgb_pre = A x + v (linearStyleTransfer.py:76-89 + the rgb conv), in the arithmetic of its inputs' dtype."""
    comp_w, comp_b, unzip_w, unzip_b, rgb_w, rgb_b = [np.asarray(t) for t in lin]
    rgb_w = rgb_w.reshape(3, 64)
    Q = rgb_w @ unzip_w.reshape(64, 32) @ np.asarray(sM).reshape(32, 32) @ np.asarray(cM).reshape(32, 32)
    A = Q @ comp_w.reshape(32, 64)
    v = Q @ comp_b - A @ np.asarray(c_mean) + rgb_w @ (unzip_b + np.asarray(s_mean)) + rgb_b
    return np.concatenate([A.reshape(-1), v])


def fold_case(seed=0):
    rng = np.random.default_rng(6000 + seed)
    sp = lambda r, c, k: sparse_int(rng, r, c, np.full(r, k), [-2, -1, 1, 2])  # noqa: E731
    sM, cM = sp(32, 32, 4), sp(32, 32, 4)
    lin = [sp(32, 64, 6), rng.integers(-3, 4, 32), sp(64, 32, 4), rng.integers(-3, 4, 64), sp(3, 64, 16), rng.integers(-3, 4, 3)]
    c_mean, s_mean = rng.integers(-3, 4, 64), rng.integers(-3, 4, 64)
    a = [np.abs(t) for t in (lin[4], lin[2], sM, cM, lin[0])]
    Qa = a[0] @ a[1] @ a[2] @ a[3]
    Aa = Qa @ a[4]
    worst = int(max(Aa.max(), (Qa @ np.abs(lin[1]) + Aa @ np.abs(c_mean) + a[0] @ (np.abs(lin[3]) + np.abs(s_mean)) + np.abs(lin[5])).max()))
    assert worst < LIMIT, "fold: %d" % worst
    assert not np.array_equal(sM @ cM, cM @ sM)
    f = lambda t: np.asarray(t, np.int64).astype(np.float32)  # noqa: E731
    want = ref_fold(sM, cM, c_mean, s_mean, lin)
    return {"sM": f(sM).reshape(-1), "cM": f(cM).reshape(-1), "c_mean": f(c_mean), "s_mean": f(s_mean), "lin": [f(t) for t in lin],
            "want": want.astype(np.float32), "bits": bits(worst), "swapped": ref_fold(cM, sM, c_mean, s_mean, lin).astype(np.float32)}


# ------------------------------------------------------------------------------------------------------------------ apply
APPLY_RANGE = 16


def apply_case(HW, seed=0):
    """Integer A, v, x: the pre-activation is an exact small integer, so sigmoid is the only inexact step -- and equal pre-activations
    must come out as equal bits."""
    rng = np.random.default_rng(7000 + seed)
    A = sparse_int(rng, 3, 64, np.full(3, 6), [-1, 1])
    v = rng.integers(-2, 3, size=3)
    x = rng.integers(-2, 3, size=(HW, 64), dtype=np.int64)
    pre = x @ A.T + v                                                       # [HW,3]
    assert np.abs(pre).max() <= APPLY_RANGE - 2
    return {"HW": HW, "x": x.astype(np.float32), "affine": np.concatenate([A.reshape(-1), v]).astype(np.float32), "pre": pre.T.copy(),
            "want": 1.0 / (1.0 + np.exp(-pre.T.astype(np.float64)))}


def ref_apply(x, affine):
    pre = np.asarray(affine[:192], np.float64).reshape(3, 64) @ np.asarray(x, np.float64).T + np.asarray(affine[192:195], np.float64)[:, None]
    return 1.0 / (1.0 + np.exp(-pre))


# ------------------------------------------------------------------------------------------------------------------ the whole decode
SEEING = 4000.0        # synth.decoder_state's contrast: the decoder "that sees" (a 1e-3 feature error moves pixels by ~7e-3)


def weight_names():
    import crnerf_amd.synth as synth
    return [k for k in synth.DECODER_SHAPES if not k.endswith(".f")]


def decode_case(HW, HWs, seed=11, gain=1.0):
    import crnerf_amd.synth as synth
    st = synth.decoder_state(seed, gain, contrast=SEEING)
    rng = np.random.default_rng(HW * 31 + HWs)
    return {"HW": HW, "HWs": HWs, "state": st, "weights": [st[k] for k in weight_names()],
            "content": rng.uniform(0, 1, (HW, 64)).astype(np.float32), "style": rng.uniform(0, 1, (HWs, 64)).astype(np.float32)}


def lrelu(v):
    return np.where(v > 0, v, 0.2 * v)


def stages64(content, style, weights, mutate=None):
    """The decode in float64, stage by stage as csrc/crossray.hip cuts it (sums, Gram sums, matrices, fold, apply).  mutate: one of
    "swap_matrices", "swap_means", "style_count" (the content Gram divided by the style's count) -- the slips the bars must see."""
    W = [np.asarray(t, np.float64).reshape(t.shape[0], -1) if t.ndim > 1 else np.asarray(t, np.float64) for t in weights]
    x, s = np.asarray(content, np.float64), np.asarray(style, np.float64)
    out = {"c_sum": x.sum(0), "s_sum": s.sum(0)}
    c_mean, s_mean = out["c_sum"] / x.shape[0], out["s_sum"] / s.shape[0]

    def gram(g, mean, w):
        h = lrelu((g - mean) @ w[0].T + w[1])
        h = lrelu(h @ w[2].T + w[3]) @ w[4].T + w[5]
        return (h.T @ h).reshape(-1)
    out["s_gram"], out["c_gram"] = gram(s, s_mean, W[0:6]), gram(x, c_mean, W[8:14])
    c_count = s.shape[0] if mutate == "style_count" else x.shape[0]
    sM, cM = ref_matrix(out["s_gram"], s.shape[0], W[6], W[7]), ref_matrix(out["c_gram"], c_count, W[14], W[15])
    if mutate == "swap_matrices":
        sM, cM = cM, sM
    if mutate == "swap_means":
        c_mean, s_mean = s_mean, c_mean
    out.update(c_mean=c_mean, s_mean=s_mean, sM=sM, cM=cM, affine=ref_fold(sM, cM, c_mean, s_mean, W[16:22]))
    out["rgb"] = ref_apply(x, out["affine"])
    return out


def oracle_rgb(case, dtype):
    """oracle.cpu_ref.crossray_decode on the case in the given torch dtype -> [3,HW] float64 numpy."""
    import torch
    from oracle import cpu_ref as O
    w = {k: torch.from_numpy(v).to(dtype) for k, v in case["state"].items()}
    x, s = torch.from_numpy(case["content"]).to(dtype), torch.from_numpy(case["style"]).to(dtype)
    with torch.no_grad():
        rgb = O.crossray_decode(w, O.feature_to_grid(x, 1, case["HW"]), O.feature_to_grid(s, 1, case["HWs"]))
    return rgb.reshape(3, -1).double().numpy()


def decode_reference(case):
    """(float64 rgb, the fp32 CPU oracle's own max error against it, the bar max(2e-5, 4 x that error))."""
    ref = oracle_rgb(case, __import__("torch").float64)
    own = float(np.abs(oracle_rgb(case, __import__("torch").float32) - ref).max())
    return ref, own, max(2e-5, 4.0 * own)


# ------------------------------------------------------------------------------------------------------------------ backward
def decode_torch(w, xc, xs, detach_stats=False):
    """oracle.cpu_ref.crossray_decode on pixel-major grids, with a switch that cuts the gradient through the two transformation matrices and the two
    means: what is left then is the direct path of x, and (full - that) is the part of a gradient that flows through the Gram chains."""
    import torch
    from oracle import cpu_ref as O
    x, s = xc.t(), xs.t()
    c_mean, s_mean = x.mean(dim=1, keepdim=True), s.mean(dim=1, keepdim=True)
    sM, cM = O.cnn_matrix(w, "snet", s - s_mean), O.cnn_matrix(w, "cnet", x - c_mean)
    if detach_stats:
        sM, cM = sM.detach(), cM.detach()
    if detach_stats and detach_stats != "matrices":
        c_mean, s_mean = c_mean.detach(), s_mean.detach()
    comp = O._conv1x1(x - c_mean, w["multi_net.compress.weight"], w["multi_net.compress.bias"])
    fused = O._conv1x1(sM @ cM @ comp, w["multi_net.unzip.weight"], w["multi_net.unzip.bias"]) + s_mean
    return torch.sigmoid(O._conv1x1(fused, w["decoder.feat_2_rgb_list.0.weight"], w["decoder.feat_2_rgb_list.0.bias"]))


D_RGB_MEAN = 3.0
"""d_rgb ~ N(3, 1), not N(0, 1).  What reaches a content pixel through the statistics is (a sum over ALL pixels of d_pre (x) x) / HW: with a zero-mean
d_rgb that sum is a random walk, the Gram part of d_content falls as 1 / sqrt(HW) against the direct path d_pre A, and at 32,801 pixels it is
0.75 x the bar of d_content itself (the conv chains' own share: 0.06 x) at every weight gain from 0.25 to 4 -- a per-element check could not see
it, whatever the weights.  A loss gradient is not zero-mean either.  With mean 3 the Gram part is 150 to 300 x the bar in every 32-pixel tile
at gain 1 (tests/test_crossray_exact_host.py asserts 10 x), the chains' own share 7 x or more."""


U24 = 2.0 ** -24


def kink_margin(x, chain):
    """min over pixels and units of |pre-activation| / delta for the two lrelu layers of one conv chain on the grid x [P,64], in float64.
    delta bounds what ANY fp32 evaluation of that pre-activation can differ from float64 by: (n + 2) 2^-24 (sum |terms| + |bias|) for its own
    n-term sum in any order (the mean's rounding is one more term), plus, for the second layer, sum_k |w_k| delta_1k handed down through the
    1-Lipschitz lrelu.  A margin above 1 means every fp32 evaluation takes the lrelu branches float64 takes.  Returns (margin, pixels below 1)."""
    w1, b1, w2, b2 = [np.asarray(t, np.float64).reshape(t.shape[0], -1) for t in chain[:4]]
    b1, b2 = b1.reshape(-1), b2.reshape(-1)
    x = np.asarray(x, np.float64)
    m = x.mean(0)
    p1 = (x - m) @ w1.T + b1
    d1 = 66 * U24 * ((np.abs(x) + np.abs(m)) @ np.abs(w1).T + np.abs(b1))
    h1 = lrelu(p1)
    p2 = h1 @ w2.T + b2
    d2 = 130 * U24 * (np.abs(h1) @ np.abs(w2).T + np.abs(b2)) + d1 @ np.abs(w2).T
    r = np.minimum((np.abs(p1) / d1).min(1), (np.abs(p2) / d2).min(1))
    return float(r.min()), np.nonzero(r <= 1.0)[0]


def off_the_kinks(x, chain, rng):
    """Move the pixels of x [P,64] whose chain has a pre-activation within delta of an lrelu kink: add a random vector (multiples of 2^-12) to the
    pixel and subtract it from a partner half a grid away, so that the channel means stay where they are and no other pixel moves.  Why: the
    gradient of lrelu jumps by a factor of 5 at 0.  In a grid of 32,801 pixels some twenty of the 6.3 million pre-activations lie within 1e-6
    of 0, and half an fp32 ulp on the mean (3e-8: two summation orders) flips one -- which moves that pixel's d_content by 3.5e-3 of the
    tensor's largest entry and the first conv's weight gradient by 2.6e-4 (measured in float64 on the CPU, and between the two entry points of
    the backward on the device).  No tolerance of the backward means anything on such a case."""
    x = np.array(x, np.float32)
    P = x.shape[0]
    for _ in range(50):
        bad = kink_margin(x, chain)[1]
        if not len(bad):
            return x
        for px in bad:
            v = (np.round(rng.uniform(-0.25, 0.25, 64) * 4096) / 4096).astype(np.float32)
            x[px] += v
            x[(px + P // 2 + 1) % P] -= v
    raise AssertionError("pixels stay on the lrelu kinks")


def backward_case(HW, HWs, seed=13, gain=1.0):
    case = decode_case(HW, HWs, seed, gain)
    rng = np.random.default_rng(HW + 7 * HWs)
    case["d_rgb"] = (rng.normal(size=(3, HW)) + D_RGB_MEAN).astype(np.float32)
    case["content"] = off_the_kinks(case["content"], case["weights"][8:12], rng)
    case["style"] = off_the_kinks(case["style"], case["weights"][0:4], rng)
    case["kink_margin"] = min(kink_margin(case["content"], case["weights"][8:12])[0], kink_margin(case["style"], case["weights"][0:4])[0])
    assert case["kink_margin"] > 1.0
    return case


def backward_reference(case, detach_stats=False):
    """float64 autograd through the oracle: (d_content, d_style, {name: gradient}) as float64 numpy."""
    import torch
    names = weight_names()
    w = {k: torch.from_numpy(case["state"][k]).double().requires_grad_(True) for k in names}
    xc, xs = torch.from_numpy(case["content"]).double().requires_grad_(True), torch.from_numpy(case["style"]).double().requires_grad_(True)
    rgb = decode_torch(w, xc, xs, detach_stats)
    (rgb * torch.from_numpy(case["d_rgb"]).double()).sum().backward()
    zero = lambda t: np.zeros(tuple(t.shape)) if t.grad is None else t.grad.numpy()  # noqa: E731
    return zero(xc), zero(xs), {k: zero(w[k]) for k in names}


def backward_bar(ref):
    """The bar of test_decoder_backward_vs_autograd_oracle (tests/test_gpu_parity.py): 2e-3 of the tensor's largest entry + 1e-8."""
    return 2e-3 * float(np.abs(ref).max()) + 1e-8


def tile_gram_part(case, detach_stats=True):
    """Per 32-pixel tile of the content grid: max |the part of d_content that flows through the Gram chains|, and the bar of d_content.
    detach_stats=True: full gradient minus the gradient with both matrices and both means detached; "matrices": the means stay attached,
    what is left is the conv chains' own per-pixel gradient (dec_bwd_chain_mfma_kernel's dxc, centred)."""
    full = backward_reference(case)[0]
    part = np.abs(full - backward_reference(case, detach_stats=detach_stats)[0]).max(1)
    n = (case["HW"] + 31) // 32
    part = np.concatenate([part, np.full(n * 32 - case["HW"], -1.0)]).reshape(n, 32).max(1)
    return part, backward_bar(full)

"""Exactly summable inputs for the appearance encoder (csrc/encoder.hip, csrc/encoder_train.hip), their float64 reference, and
the certificate that makes "bit for bit" a fair demand.  Shared by tests/test_encoder_exact_host.py (CPU) and
tests/test_gpu_encoder_exact.py; imports numpy, torch and the oracle only -- never the product package.

THE IDEA.  A sum of fp32 numbers that are all multiples of one power of two q, and whose absolute values add up to A < 2^24 q, is
exact in fp32 in EVERY order: each partial sum is a multiple of q below 2^24 q, so it has at most 24 significant bits.  Fused or
not, on the vector ALU or in v_mfma_f32_32x32x2_f32, split over waves or chunks, a kernel that forms the right terms gives the
float64 result to the bit -- and one that takes a wrong index does not.  No tolerance is involved.

THE INPUTS.  Image: small non-negative integers.  Weights: non-negative and dyadic -- "selection" layers hold ONE unit weight per
output row, at (channel, tap) positions that rotate with the case so that all cases together touch every tap of every layer; one
layer per case is "dense" (four non-zeros per row from {1, 2} * 2^-s, s <= 2).  Biases: k/4, k = 1..4.  So every pre-activation
is > 0, LeakyReLU is the identity, its derivative 1, and the inexact factor 0.2 never enters a sum.  Cotangent: sparse integers in
-2..2.  Integer images tie inside 2 x 2 max-pool windows all the time; the "blocks" cases make most windows tie in all four entries.

THE TIE RULE.  MaxPool2d's backward sends the gradient to the FIRST maximum of the window in scan order (row-major: (0,0), (0,1),
(1,0), (1,1)).  That is ATen's rule (max_pool2d_with_indices keeps the first index whose value is greater than the running
maximum, or NaN), enc_maxpool2_bwd_kernel restates it, and first_maximum_rule_holds() checks it on a 2 x 2 tie.

LIMITS.  The negative LeakyReLU branch never occurs inside the chain (sign_case() reaches it at the last layer, forward only), and
AdaptiveAvgPool2d windows must have areas 1, 2 or 4 (a division by 3, 6 or 9 is inexact): quarter-resolution maps of at most 32,
or 48 or 64 rows.  Those stay with the tolerance tests.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

from oracle import cpu_ref as O

CIN = (3, 3, 64, 64, 128, 128, 128)
COUT = (3, 64, 64, 128, 128, 128, 64)
TAPS = (1, 9, 9, 9, 9, 9, 1)
NAMES = ["conv%d.%s" % (l, t) for l in range(1, 8) for t in ("weight", "bias")]
ROTATIONS = 9            # 9 * 128 rows = the 1,152 (channel, tap) columns of conv5 / conv6

# name, H, W, seed, rotation, dense layer (2..7), image bits, cotangent density, image kind
_SPECS = [
    ("8x8", 8, 8, 1, 0, 2, 3, 0.10, "noise"),            # H4 = W4 = 2: every quarter-resolution pixel is both "row 1" and "row n-2"
    ("11x9", 11, 9, 2, 1, 3, 3, 0.10, "noise"),          # the same with odd H, W
    ("12x15", 12, 15, 3, 2, 4, 3, 0.10, "noise"),        # H4 = W4 = 3: the middle pixel collects both mirrors
    ("14x13", 14, 13, 4, 3, 5, 3, 0.10, "noise"),        # odd H2 = 7, W2 = 6
    ("10x20", 10, 20, 5, 4, 6, 3, 0.10, "noise"),        # odd H2
    ("9x23", 9, 23, 6, 5, 7, 3, 0.10, "noise"),
    ("24x40", 24, 40, 7, 6, 2, 3, 0.10, "noise"),
    ("21x37", 21, 37, 8, 7, 3, 3, 0.10, "noise"),        # W % 8 != 0; H*W % 32 != 0 on every level
    ("130x128", 130, 128, 9, 8, 5, 2, 0.10, "noise"),    # H4 = 32; the largest weight-gradient sums
    ("192x8", 192, 8, 10, 0, 6, 3, 0.10, "noise"),       # H4 = 48: averaging windows of two rows, overlapping; W4 = 2
    ("256x16", 256, 16, 11, 1, 4, 3, 0.10, "noise"),     # H4 = 64: windows of two rows; W4 = 4
    ("24x40-blocks", 24, 40, 12, 2, 7, 3, 0.10, "blocks"),   # piecewise-constant image: four-way ties in most pooling windows
    ("21x37-blocks", 21, 37, 13, 3, 6, 3, 0.25, "blocks"),
    ("64x40", 64, 40, 14, 4, 3, 3, 0.10, "noise"),       # the row-band shapes (with 256x16)
    ("128x24", 128, 24, 15, 5, 5, 3, 0.10, "noise"),
]
CASE_NAMES = [s[0] for s in _SPECS]
BAND_CASES = [("64x40", 2), ("64x40", 4), ("64x40", 8), ("128x24", 2), ("128x24", 4), ("128x24", 8), ("256x16", 2), ("256x16", 4), ("256x16", 8)]
PARITY_SHAPES = [(8, 8), (11, 9), (12, 15), (14, 13), (10, 20), (9, 23), (21, 37), (176, 8)]   # (176, 8): H4 = 44, averaging windows of 3 rows


def _column_order(layer):
    return np.random.default_rng(1000 + layer).permutation(CIN[layer] * TAPS[layer])


def make_weights(seed, rotation, dense):
    """The 14 tensors (float64 numpy, state_dict names).  Row o of a selection layer holds a 1 at column order[(rotation * cout + o) % K] of its
    [cout, cin * taps] matrix; the dense layer keeps that column and adds three more, each {1, 2} * 2^-{0, 1, 2}."""
    rng = np.random.default_rng(seed)
    w = {}
    for l in range(7):
        K, co = CIN[l] * TAPS[l], COUT[l]
        m = np.zeros((co, K))
        sel = _column_order(l)[(rotation * co + np.arange(co)) % K]
        m[np.arange(co), sel] = 1.0
        if l + 1 == dense:
            for o in range(co):
                for k in [sel[o]] + list(rng.choice(K, 3, replace=False)):
                    m[o, k] = float(rng.integers(1, 3)) * 2.0 ** -int(rng.integers(0, 3))
        k = 3 if TAPS[l] == 9 else 1
        w["conv%d.weight" % (l + 1)] = m.reshape(co, CIN[l], k, k)
        w["conv%d.bias" % (l + 1)] = rng.integers(1, 5, co) / 4.0
    return w


_cache = {}


def get_case(name):
    """{"name", "H", "W", "img" [3,H,W], "weights" {name: array}, "cot" [1024,64] (pixel-major, as ops.encoder_backward takes it)}, float64 numpy."""
    if name not in _cache:
        _, H, W, seed, rot, dense, bits, density, kind = _SPECS[CASE_NAMES.index(name)]
        rng = np.random.default_rng(seed)
        if kind == "blocks":   # 4 x 4 blocks of one value, shifted by one pixel so that block edges cross pooling windows too
            coarse = rng.integers(0, 2 ** bits, (3, H // 4 + 2, W // 4 + 2))
            img = np.kron(coarse, np.ones((1, 4, 4), dtype=np.int64))[:, 1:H + 1, 1:W + 1]
        else:
            img = rng.integers(0, 2 ** bits, (3, H, W))
        cot = rng.integers(-2, 3, (1024, 64)) * (rng.random((1024, 64)) < density)
        _cache[name] = {"name": name, "H": H, "W": W, "dense": dense, "img": img.astype(np.float64), "weights": make_weights(seed, rot, dense),
                        "cot": cot.astype(np.float64)}
    return _cache[name]


def sign_case(case):
    """The same inputs with conv7's bias moved down to about the median of each output channel's pre-activation: about
    half of conv7's outputs turn negative.  Returns (case', expected [1024,64] float32): float32(0.2) * float32(v) where v < 0 -- v itself is
    exact, so that product is rounded once, which is what lrelu() in enc_gemm_nt_kernel<true>'s epilogue does."""
    ref = reference(case)
    b7 = case["weights"]["conv7.bias"]
    pre = ref["out"].numpy()                                   # positive branch: the pre-activation itself
    shift = np.empty(64)
    for o in range(64):                                        # per channel: the threshold between two of its values that splits it most evenly
        u = np.unique(pre[:, o])
        below = np.array([(pre[:, o] < t).mean() for t in u])
        shift[o] = u[np.argmin(np.abs(below - 0.5))] - 2.0 ** -9   # (every pre-activation is a multiple of 2^-8: no output lands on zero)
    v = pre - shift[None, :]
    assert (v != 0).all() and 0.25 < (v < 0).mean() < 0.75, float((v < 0).mean())
    v32 = v.astype(np.float32)
    assert (v32.astype(np.float64) == v).all()
    want = np.where(v32 > 0, v32, np.float32(0.2) * v32).astype(np.float32)
    weights = dict(case["weights"])
    weights["conv7.bias"] = b7 - shift
    assert (weights["conv7.bias"].astype(np.float32).astype(np.float64) == weights["conv7.bias"]).all()
    return dict(case, weights=weights, name=case["name"] + "-sign"), want


# ------------------------------------------------------------------------------------------------------------------ reference
def cot_nchw(case, dtype, rows=None):
    """The cotangent in the reference's layout [1,64,32,32]; rows = (o0, o1): only those rows of the 32 x 32 grid, zero elsewhere (a row band)."""
    c = torch.tensor(case["cot"], dtype=dtype).view(32, 32, 64).permute(2, 0, 1)[None].clone()
    if rows is not None:
        c[:, :, :rows[0]] = 0
        c[:, :, rows[1]:] = 0
    return c


def pixel_major(out):
    return out.detach()[0].permute(1, 2, 0).reshape(1024, 64).contiguous()


def reference(case, dtype=torch.float64, forward=O.encoder_forward, bands=None):
    """oracle.cpu_ref.encoder_forward (or another restatement) + torch autograd -> {"out" [1024,64], "grads" (14, NAMES' order), "d_img" [3,H,W]}.
    bands: a list of (o0, o1) -> additionally "bands": the same gradients for the cotangent restricted to each band's rows."""
    w = {k: torch.tensor(v, dtype=dtype).requires_grad_() for k, v in case["weights"].items()}
    img = torch.tensor(case["img"], dtype=dtype)[None].requires_grad_()
    out = forward(w, img)
    leaves = [w[n] for n in NAMES] + [img]

    def grads(cot):
        g = torch.autograd.grad((out * cot).sum(), leaves, retain_graph=True)
        return {"grads": list(g[:14]), "d_img": g[14][0]}
    res = grads(cot_nchw(case, dtype))
    res["out"] = pixel_major(out)
    if bands is not None:
        res["bands"] = [grads(cot_nchw(case, dtype, b)) for b in bands]
    return res


def encoder_forward_im2col(d, img, seed=0):
    """encoder_sameoutputsize.forward with every convolution as ONE matrix product over the patch matrix, the K axis (cin * taps) of both operands
    shuffled: a second summation order for the fp32 CPU run (and, through autograd, for its gradients)."""
    gen = torch.Generator().manual_seed(seed)

    def conv(x, i, act=True):
        wt, b = d["conv%d.weight" % i], d["conv%d.bias" % i]
        _, _, H, W = x.shape
        if wt.shape[-1] == 3:
            x = F.pad(x, (1, 1, 1, 1), mode="reflect")
        cols = F.unfold(x, wt.shape[-1])[0]                               # [cin * taps, H * W]
        order = torch.randperm(cols.shape[0], generator=gen)
        y = (wt.reshape(wt.shape[0], -1)[:, order] @ cols[order] + b[:, None]).view(1, wt.shape[0], H, W)
        return F.leaky_relu(y, 0.2) if act else y
    x = conv(img, 1, act=False)
    x = F.max_pool2d(conv(conv(x, 2), 3), 2, 2)
    x = F.max_pool2d(conv(conv(x, 4), 5), 2, 2)
    x = F.adaptive_avg_pool2d(conv(x, 6), 32)
    return conv(x, 7)


def first_maximum_rule_holds():
    """ATen routes a tied 2 x 2 window's gradient to its first entry in scan order -- in float64 and float32."""
    for dtype in (torch.float64, torch.float32):
        for vals, first in (([[5, 5], [5, 5]], 0), ([[1, 5], [5, 5]], 1), ([[1, 2], [5, 5]], 2), ([[5, 1], [5, 1]], 0)):
            x = torch.tensor(vals, dtype=dtype).view(1, 1, 2, 2).requires_grad_()
            F.max_pool2d(x, 2, 2).sum().backward()
            if x.grad.flatten().tolist() != [1.0 if k == first else 0.0 for k in range(4)]:
                return False
    return True


# ------------------------------------------------------------------------------------------------------------------ certificate
def pool_windows(n_in, S=32, floor_end=False):
    """AdaptiveAvgPool2d(S)'s windows along one axis: [floor(o n / S), ceil((o + 1) n / S)) for o = 0..S-1."""
    return [((o * n_in) // S, ((o + 1) * n_in) // S if floor_end else ((o + 1) * n_in + S - 1) // S) for o in range(S)]


def quantum(t):
    """The largest power of two that divides every entry (inf for an all-zero tensor)."""
    a = np.abs(np.asarray(t, dtype=np.float64)).ravel()
    a = a[a != 0]
    if a.size == 0:
        return math.inf
    n = a * 2.0 ** 40
    assert (n == np.round(n)).all() and n.max() < 2.0 ** 62, "entries must be multiples of 2^-40 below 2^22"
    n = n.astype(np.int64)
    return float((n & -n).min()) / 2.0 ** 40


def certificate(case, rows=None, forward_only=False):
    """Walks the network and its backward in float64 and bounds every sum that any kernel forms: with q a power of two dividing all of the sum's
    terms (the product of its operands' quanta: a lower bound of the largest such q, so the bound errs on the safe side) and A = sum |terms|,
    it needs A < 2^24 q.  A is taken over the FULL sum behind an output element (for the data gradient of a 3x3 layer: over cout, taps and the
    mirrored copies at once), which bounds every partial sum inside it -- the GEMM's, the wave split's, the chunk partials', col2im's.
    Returns {sum name: log2(max A / q)}, all below 24, or raises AssertionError.  rows = (o0, o1): for the cotangent of one row band.
    forward_only: the forward sums alone, and conv7's pre-activation may be negative (sign_case); "conv6": up to conv6 (a row band's own rows).
    Also asserts what the construction promises: every pre-activation > 0, pooling window areas in {1, 2, 4}."""
    T = lambda v: torch.tensor(v, dtype=torch.float64)  # noqa: E731
    w = {k: T(v) for k, v in case["weights"].items()}
    x0 = T(case["img"])[None].requires_grad_()
    bits = {}

    def note(key, A, q):
        A = float(A)
        bits[key] = -math.inf if A == 0.0 else math.log2(A / q)
        assert bits[key] < 24.0, "%s: %s needs %.1f bits" % (case["name"], key, bits[key])

    def pad(x, i):
        return F.pad(x, (1, 1, 1, 1), mode="reflect") if TAPS[i - 1] == 9 else x

    ins, outs = {}, {}

    def conv(x, i):
        wt, b = w["conv%d.weight" % i], w["conv%d.bias" % i]
        y = F.conv2d(pad(x, i), wt, b)
        with torch.no_grad():
            note("conv%d forward" % i, F.conv2d(pad(x, i).abs(), wt.abs(), b.abs()).max(), min(quantum(x.detach()) * quantum(wt), quantum(b)))
            assert i == 1 or (i == 7 and forward_only) or bool((y > 0).all()), "conv%d has a non-positive pre-activation" % i
        y.retain_grad()
        ins[i], outs[i] = x, y
        return y
    h = conv(x0, 1)
    h = F.max_pool2d(F.leaky_relu(conv(F.leaky_relu(conv(h, 2), 0.2), 3), 0.2), 2, 2)
    h = F.max_pool2d(F.leaky_relu(conv(F.leaky_relu(conv(h, 4), 0.2), 5), 0.2), 2, 2)
    y6 = F.leaky_relu(conv(h, 6), 0.2)
    if forward_only == "conv6":
        return bits
    H4, W4 = y6.shape[-2:]
    area = torch.tensor([[(y1 - y0) * (x1 - x0) for (x0, x1) in pool_windows(W4)] for (y0, y1) in pool_windows(H4)], dtype=torch.float64)
    assert set(area.flatten().tolist()) <= {1.0, 2.0, 4.0}, "averaging windows of area %s divide inexactly" % sorted(set(area.flatten().tolist()))
    p6 = F.adaptive_avg_pool2d(y6, 32)
    p6.retain_grad()
    with torch.no_grad():
        note("avgpool forward", (F.adaptive_avg_pool2d(y6.abs(), 32) * area).max(), quantum(y6.detach()))
    out = F.leaky_relu(conv(p6, 7), 0.2)
    assert torch.equal(out.detach(), O.encoder_forward(w, x0.detach())), "the certificate walks another network than the oracle"
    if forward_only:
        return bits
    (out * cot_nchw(case, torch.float64, rows)).sum().backward()
    # backward: g = the gradient at each convolution's output (LeakyReLU's derivative is 1 everywhere)
    for i in range(7, 0, -1):
        g, xin, wt = outs[i].grad, ins[i].detach(), w["conv%d.weight" % i]
        qg = quantum(g)
        note("conv%d bias gradient" % i, g.abs().sum(dim=(0, 2, 3)).max(), qg)
        wv = torch.zeros_like(wt).requires_grad_()
        note("conv%d weight gradient" % i, torch.autograd.grad((F.conv2d(pad(xin, i).abs(), wv) * g.abs()).sum(), wv)[0].max(), qg * quantum(xin))
        xv = torch.zeros_like(xin).requires_grad_()
        note("conv%d data gradient" % i, torch.autograd.grad((F.conv2d(pad(xv, i), wt.abs()) * g.abs()).sum(), xv)[0].max(), qg * quantum(wt))
        if i == 7:
            yv = torch.zeros_like(y6).requires_grad_()
            note("avgpool backward", torch.autograd.grad((F.adaptive_avg_pool2d(yv, 32) * p6.grad.abs()).sum(), yv)[0].max(), quantum(p6.grad) / 4.0)
    return bits


# ------------------------------------------------------------------------------------------------------------------ index emulation
MUTANTS = ("reflect_high", "last_maximum", "floor_window_end", "drop_row_n_minus_2", "clamp_early")


class Emulation:
    """The encoder's forward and backward in numpy float64, pixel-major like the kernels, with the kernels' own index arithmetic spelled out:
    reflect(), the column clamp of conv_kernel's pixel groups, the pooling windows, the tie rule of the max-pool backward and the ty[] / tx[]
    membership lists of the reflection adjoint.  mutant = one of MUTANTS breaks exactly one of them:
      reflect_high        reflect(i, n) = 2n - 1 - i for i >= n (the edge pixel itself instead of its inner neighbour)
      last_maximum        the max-pool backward keeps the LAST maximum of a window (v >= best)
      floor_window_end    the averaging window's last row is floor((o + 1) H4 / 32) instead of ceil (forward and backward)
      drop_row_n_minus_2  row H - 2 no longer collects the gradient of the mirrored padded row H
      clamp_early         conv_kernel's column clamp engages one column early: x < W - 1 ? x : W - 2 (see clamp_note)
    """
    clamp_note = ("conv_kernel computes `x0 + j < W ? x0 + j : W - 1` only to keep the idle lanes of the last pixel group readable; their results are "
                  "dropped at the store, so replacing the VALUE W - 1 by W - 2 alone changes no output of any input (it is not a bug either). "
                  "The mutant here moves bound and value together, which is the nearest error that can reach an output.")

    def __init__(self, mutant=None):
        assert mutant is None or mutant in MUTANTS
        self.m = mutant

    def reflect(self, i, n):
        hi = 2 * n - 1 - i if self.m == "reflect_high" else 2 * n - 2 - i
        return np.where(i < 0, -i, np.where(i >= n, hi, i))

    def patches(self, x, clamp=False):
        """x [H,W,C] -> X [H*W, C*9], X[px][c*9 + tap] = x[reflect(py + ky - 1)][reflect(col(pxx) + kx - 1)][c]"""
        H, W, C = x.shape
        col = np.arange(W)
        if clamp and self.m == "clamp_early":
            col = np.where(col < W - 1, col, W - 2)
        X = np.empty((H, W, C, 9))
        for ky in range(3):
            ry = self.reflect(np.arange(H) + ky - 1, H)
            for kx in range(3):
                X[:, :, :, ky * 3 + kx] = x[ry][:, self.reflect(col + kx - 1, W)]
        return X.reshape(H * W, C * 9)

    def members(self, n, rows):
        """(p, q, k): padded coordinate t in {p, -1 if p == 1, n if p == n - 2}, patch q = t - k + 1 inside the map"""
        out = []
        for p in range(n):
            ts = [p] + ([-1] if p == 1 else []) + ([n] if p == n - 2 and not (rows and self.m == "drop_row_n_minus_2") else [])
            out += [(p, t - k + 1, k) for t in ts for k in range(3) if 0 <= t - k + 1 < n]
        return out

    def col2im(self, dX, H, W, C):
        d5 = dX.reshape(H, W, C, 3, 3)
        tmp = np.zeros((H, W, C, 3))
        for p, q, k in self.members(H, True):
            tmp[p] += d5[q, :, :, k, :]
        out = np.zeros((H, W, C))
        for p, q, k in self.members(W, False):
            out[:, p] += tmp[:, q, :, k]
        return out

    @staticmethod
    def pool(x):
        H, W, _ = x.shape
        v = x[:H // 2 * 2, :W // 2 * 2]
        return np.maximum(np.maximum(v[0::2, 0::2], v[0::2, 1::2]), np.maximum(v[1::2, 0::2], v[1::2, 1::2]))

    def pool_bwd(self, x, d):
        H, W, _ = x.shape
        Ho, Wo = H // 2, W // 2
        v = [x[dy:2 * Ho:2, dx:2 * Wo:2] for dy in (0, 1) for dx in (0, 1)]     # scan order
        best, bv = np.zeros(v[0].shape, dtype=np.int64), v[0].copy()
        for k in range(1, 4):
            take = v[k] >= bv if self.m == "last_maximum" else v[k] > bv
            best, bv = np.where(take, k, best), np.where(take, v[k], bv)
        out = np.zeros_like(x)                                                  # (an odd last row / column lies in no window)
        for k, (dy, dx) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
            out[dy:2 * Ho:2, dx:2 * Wo:2] = np.where(best == k, d, 0.0)
        return out

    def run(self, case):
        lr = lambda v: np.where(v > 0, v, 0.2 * v)          # noqa: E731
        dl = lambda v: np.where(v > 0, 1.0, 0.2)            # noqa: E731
        wt = lambda i: case["weights"]["conv%d.weight" % i].reshape(COUT[i - 1], -1)   # noqa: E731
        b = lambda i: case["weights"]["conv%d.bias" % i]    # noqa: E731
        H, W = case["H"], case["W"]
        floor_end = self.m == "floor_window_end"
        a0 = case["img"].transpose(1, 2, 0).reshape(H * W, 3)
        y1 = a0 @ wt(1).T + b(1)
        X, y, shape = {}, {1: y1}, {2: (H, W), 3: (H, W), 4: (H // 2, W // 2), 5: (H // 2, W // 2), 6: (H // 4, W // 4)}
        cur = y1.reshape(H, W, 3)
        for i in range(2, 7):
            if i in (4, 6):
                cur = self.pool(cur)
            X[i] = self.patches(cur, clamp=(i == 2))                            # conv2 runs on conv_kernel<9>, the others on the patch-matrix GEMM
            y[i] = lr(X[i] @ wt(i).T + b(i))
            cur = y[i].reshape(shape[i] + (COUT[i - 1],))
        H4, W4 = shape[6]
        wy, wx = pool_windows(H4, floor_end=floor_end), pool_windows(W4)
        p6 = np.zeros((32, 32, 128))
        with np.errstate(invalid="ignore", divide="ignore"):
            for oy, (r0, r1) in enumerate(wy):
                for ox, (c0, c1) in enumerate(wx):
                    p6[oy, ox] = cur[r0:r1, c0:c1].sum(axis=(0, 1)) / float((r1 - r0) * (c1 - c0))
        p6 = p6.reshape(1024, 128)
        out = lr(p6 @ wt(7).T + b(7))
        grads = {}
        g = case["cot"] * dl(out)
        grads[7] = (g.T @ p6, g.sum(0))
        dp6 = (g @ wt(7)).reshape(32, 32, 128)
        d = np.zeros((H4, W4, 128))
        with np.errstate(invalid="ignore", divide="ignore"):
            for oy, (r0, r1) in enumerate(wy):
                for ox, (c0, c1) in enumerate(wx):
                    d[r0:r1, c0:c1] += dp6[oy, ox] / float((r1 - r0) * (c1 - c0))
        for i in range(6, 1, -1):
            h, ww = shape[i]
            g = d.reshape(h * ww, COUT[i - 1]) * dl(y[i])
            grads[i] = (g.T @ X[i], g.sum(0))
            d = self.col2im(g @ wt(i), h, ww, CIN[i - 1])
            if i in (6, 4):
                hs, wss = shape[i - 1]
                d = self.pool_bwd(y[i - 1].reshape(hs, wss, COUT[i - 2]), d)
        g = d.reshape(H * W, 3)
        grads[1] = (g.T @ a0, g.sum(0))
        d_img = (g @ wt(1)).T.reshape(3, H, W)
        flat = [t for i in range(1, 8) for t in (grads[i][0].reshape(case["weights"]["conv%d.weight" % i].shape), grads[i][1])]
        return {"out": out, "grads": flat, "d_img": d_img}


def differs(a, b):
    """Names of the outputs of two runs (reference() or Emulation.run()) that are not equal bit for bit (NaN counts as different)."""
    arr = lambda t: t.detach().numpy() if torch.is_tensor(t) else np.asarray(t)   # noqa: E731
    bad = [] if np.array_equal(arr(a["out"]), arr(b["out"])) else ["out"]
    bad += [n for n, p, q in zip(NAMES, a["grads"], b["grads"]) if not np.array_equal(arr(p), arr(q))]
    return bad + ([] if np.array_equal(arr(a["d_img"]), arr(b["d_img"])) else ["d_img"])

"""Exactly summable operands for the MLP data gradients (mlp_backward16_kernel in csrc/mlp_train16.hip, mlp_backward_h2_kernel, mlp_backward_x3_kernel),
their float64 reference, the certificate that makes "bit for bit" a fair demand, the relu-bit map of the saved state and numpy emulations of the
kernels' index arithmetic.  Shared by tests/test_dgrad_exact_host.py (CPU) and tests/test_gpu_dgrad_exact.py; imports numpy and torch only -- never
the product package.  The byte offsets of the saved state and of the scratch buffer come from tests/_wgrad_cases.py.

THE IDEA.  Per point, the backward-data pass is a chain of eleven short sums:
    d_rgb  = d_out[:, :64] * f (1 - f)                       f = out[:, :64]
    d_sig  = d_out[:, 64] * (1 - exp(-out[:, 64]))
    slot 9 = (d_rgb . W_rgb) o bits_9                         128 columns          (slot: the delta row of that number in the scratch buffer)
    slot 8 = slot 9 . W_dir[:, :256]                          linear: no mask
    slot 7 = (slot 8 . W_final + d_sig w_sigma) o bits_7
    slot l - 1 = (slot l . W_{l+1}) o bits_{l-1}, l = 7..1    W_5: its columns 93.. (the skip hands xyz on in columns 0..92)
A sum has at most 256 + 1 terms and runs over FEATURES, so whatever holds for one point holds for any number of them.  If every term of a sum is a
multiple of one power of two q and sum |terms| < 2^24 q, every partial sum in any order is an fp32 number: the fp32 MFMA, the two-piece fp16 and
the three-piece bf16 products (as long as their pieces are exact, fair_cores()) all give the float64 result to the bit, and a kernel that reads a
relu bit of the neighbouring lane group, masks the linear slot, misses the sigma head in one tile or stores a piece into the wrong row does not.

THE DATA.  Weights: sparse (k non-zeros per column, at most 3 k per row), entries +-1, +-2, +-1/2 (w_sigma: +-1/16, +-1/8), every column non-zero,
neighbouring columns with different supports; the xyz / dir columns that the chain does not read are filled like the others.  out[:, :64] in
{0, 1/4, 1/2, 3/4, 1} (f (1 - f) in {0, 3/16, 1/4}: exact), out[:, 64] in {0, 200} (softplus' = 1 - exp(-sigma) is 0 or 1 in any expf), d_out small
integers, half of them zero, one point in eight all zero.  The relu bits are written directly, 64-bit random words: slot 8 all zero (it is linear: a
kernel that applies the word zeroes the chain), bits 32..63 of slot 9 (features beyond 128) the complement of bits 0..31.
EDGE MARKS.  Regular points carry |d_out| <= gm.  The last point of every 16-, 32- and 128-point unit carries +-(gm + 1) in every column, with a
sign pattern of its own per unit size, the last point of the case +-(gm + 2), point 0 +-(gm + 3) (lanes past the end read row 0); marked points
have f in {1/4, 1/2}, sigma = 200, so none of their d_rgb / d_sig vanishes.

THE FAMILIES.  narrow: one non-zero per column (+-1, +-2, +-1/2) except static_rgb and xyz_encoding_final (two, +-1), |d_out| <= 1: every delta has
at most 8 significant bits (one bf16 piece, one fp16 piece under the point's scale).  wide3: three non-zeros (+-1) per column everywhere,
|d_out| <= 2: sums of many terms; masks and signs keep them near 10 bits (second bf16 pieces).  wide12 / wide18: narrow's shape with +-1 only
and |d_out| up to 2^12 / 2^18: 16 / 22 bits -- second and third bf16 pieces, second fp16 pieces, and for wide18 rows that two fp16 pieces under
one scale no longer hold (fair_cores() then leaves h2 out).
"""
import math

import numpy as np
import torch

import _wgrad_cases as _WG
from _wgrad_cases import (DIR, FEAT, SLOTS, TENSOR_NAMES, W, XYZ, first_difference, layout, pieces_bf16, range_word,  # noqa: F401  (re-exported)
                          unpack_state)

CORES = ("fp32", "h2", "x3")
SHAPES = ([(256, 93), (256,)] + [(256, 256), (256,)] * 3 + [(256, 349), (256,)] + [(256, 256), (256,)] * 3
          + [(256, 256), (256,), (1, 256), (1,), (128, 283), (128,), (64, 128), (64,)])
LAYERS = ["xyz_encoding_%d.0" % i for i in range(1, 9)] + ["xyz_encoding_final", "static_sigma.0", "dir_encoding.0", "static_rgb.0"]
# k: non-zeros per column of a layer's weight (default, then the exceptions); vals: the magnitudes drawn; gm: the largest regular |d_out|
_TWO = {"static_rgb.0": 2, "xyz_encoding_final": 2}
FAMILIES = {
    "narrow": dict(k=1, k_of=_TWO, vals=(1.0, 2.0, 0.5), gm=1),
    "wide3": dict(k=3, k_of={}, vals=(1.0,), gm=2),
    "wide12": dict(k=1, k_of=_TWO, vals=(1.0,), gm=2 ** 12 - 4),
    "wide18": dict(k=1, k_of=_TWO, vals=(1.0,), gm=2 ** 18 - 4),
}
SIGMA_ON = 200.0
SPLIT_SLACK = 1.0 + 2.0 ** -6         # sum |pieces| of a round-to-nearest split exceeds |value| by less than this factor


# ------------------------------------------------------------------------------------------------------------------ construction
def _sparse(n_out, n_in, k, vals, gen):
    """[n_out, n_in]: k non-zeros per column, in rows pi[(i + 37 j) % n_out], j < k (pi: a permutation) -- at most ceil(n_in / n_out) k per row"""
    w = torch.zeros(n_out, n_in, dtype=torch.float32)
    pi = torch.randperm(n_out, generator=gen)
    col = torch.arange(n_in)
    v = torch.tensor(vals, dtype=torch.float32)
    for j in range(k):
        mag = v[torch.randint(0, len(vals), (n_in,), generator=gen)]
        sgn = (torch.randint(0, 2, (n_in,), generator=gen) * 2 - 1).float()
        w[pi[(col + 37 * j) % n_out], col] = mag * sgn
    return w


def make_weights(family, seed):
    """The 24 tensors (TENSOR_NAMES order, fp32, CPU).  Biases: multiples of 1/4 (the data gradient does not read them)."""
    f = FAMILIES[family]
    gen = torch.Generator()
    gen.manual_seed(seed * 7919 + sorted(FAMILIES).index(family))
    out = []
    for name, (n_out, n_in) in zip(LAYERS, SHAPES[0::2]):
        k = f["k_of"].get(name, f["k"])
        if name == "static_sigma.0":
            c = torch.arange(n_in)
            w = (((c & 1) + 1).float() / 16.0 * (torch.randint(0, 2, (n_in,), generator=gen) * 2 - 1).float())[None]
        else:
            w = _sparse(n_out, n_in, k, f["vals"] if k == 1 else (1.0,), gen)
        out += [w, torch.randint(-4, 5, (n_out,), generator=gen).float() / 4.0]
    return out


def _pattern(c, kind):
    return 1 - 2 * ((c >> kind) & 1)


def make_case(P, family, seed, device="cpu"):
    """{"P", "family", "weights" (24), "out" [P,65], "d_out" [P,65], "bits" [10,P,4] int64}: tensors on `device` (the random streams of two devices
    differ; every case is certified by certificate(), which runs on either)."""
    f = FAMILIES[family]
    gm = f["gm"]
    gen = torch.Generator(device=device)
    gen.manual_seed(seed * 1000003 + P)
    ri = lambda lo, hi, shape: torch.randint(lo, hi, shape, generator=gen, device=device, dtype=torch.int64)   # noqa: E731
    out = torch.empty(P, 65, dtype=torch.float32, device=device)
    out[:, :64] = ri(0, 5, (P, 64)).float() / 4.0
    out[:, 64] = ri(0, 2, (P,)).float() * SIGMA_ON
    d = ri(1, gm + 1, (P, 65)) * ri(0, 2, (P, 65)) * (ri(0, 2, (P, 65)) * 2 - 1)
    d[ri(0, 8, (P,)) == 0] = 0                                                       # rows of all zeros: the split cores' zero-vector path
    c = torch.arange(65, device=device)
    p = torch.arange(P, device=device)
    marked = torch.zeros(P, dtype=torch.bool, device=device)
    for unit, kind in ((16, 0), (32, 1), (128, 2)):
        rows = p % unit == unit - 1
        d[rows] = (gm + 1) * _pattern(c, kind)
        marked |= rows
    d[P - 1] = (gm + 2) * _pattern(c, 0) * _pattern(c, 2)
    d[0] = (gm + 3) * _pattern(c, 1) * _pattern(c, 2)
    marked[P - 1] = marked[0] = True
    out[marked, :64] = (0.25 + 0.25 * ((c[:64] + p[marked][:, None]) & 1)).float()
    out[marked, 64] = SIGMA_ON
    lo, hi = ri(0, 2 ** 32, (SLOTS, P, 4)), ri(0, 2 ** 32, (SLOTS, P, 4))
    hi[9] = ~lo[9] & 0xffffffff
    bits = (hi << 32) | lo
    bits[8] = 0
    return {"P": P, "family": family, "weights": [w.to(device) for w in make_weights(family, seed)], "out": out, "d_out": d.float(), "bits": bits}


def to_device(case, dev):
    return {k: ([t.to(dev) for t in v] if isinstance(v, list) else v.to(dev) if torch.is_tensor(v) else v) for k, v in case.items()}


def state_dict(case):
    return dict(zip(TENSOR_NAMES, case["weights"]))


# ------------------------------------------------------------------------------------------------------------------ the relu-bit map
def _bit_places(device):
    c = torch.arange(W, device=device)
    return (c >> 2) & 3, 4 * (c >> 4) + (c & 3)              # word g, bit 4 T + r of feature c = 16 T + 4 g + r  (csrc/mlp_train16.h)


def bits_to_mask(words):
    """[P,4] int64 -> [P,256] bool: feature 16 T + 4 g + r <-> bit 4 T + r of word g"""
    g, k = _bit_places(words.device)
    return ((words[:, g] >> k) & 1).bool()


def mask_to_bits(mask):
    """The inverse, for a [P, n <= 256] bool (the missing features count as inactive)."""
    P, n = mask.shape
    full = torch.zeros(P, W, dtype=torch.int64, device=mask.device)
    full[:, :n] = mask.long()
    g, k = _bit_places(mask.device)
    words = torch.zeros(P, 4, dtype=torch.int64, device=mask.device)
    for gg in range(4):
        sel = g == gg
        words[:, gg] = (full[:, sel] << k[sel]).sum(1)      # distinct bits: the sum is their union (bit 63 wraps to the sign, as it should)
    return words


def pack_bits(acts_buf, bits, P):
    """Writes the words into a saved-state buffer (uint8) at masks[slot][point][g]."""
    m0 = layout(P)["masks"]
    acts_buf[m0:m0 + SLOTS * P * 32].view(torch.int64).view(SLOTS, P, 4).copy_(bits)


def unpack_bits(acts_buf, P):
    m0 = layout(P)["masks"]
    return acts_buf[m0:m0 + SLOTS * P * 32].view(torch.int64).view(SLOTS, P, 4).clone()


# ------------------------------------------------------------------------------------------------------------------ reference
def _w(case, name):
    return case["weights"][TENSOR_NAMES.index(name + ".weight")]


def chain_steps(case):
    """The matrices of the chain, in the order it runs: (slot written, W [rows = the source's features, cols = the slot's features], masked)."""
    steps = [(9, _w(case, "static_rgb.0"), True), (8, _w(case, "dir_encoding.0")[:, :W], False), (7, _w(case, "xyz_encoding_final"), True)]
    for l in range(7, 0, -1):                                # slot l - 1 through xyz_encoding_{l+1}
        w = _w(case, "xyz_encoding_%d.0" % (l + 1))
        steps.append((l - 1, w[:, XYZ:] if l + 1 == 5 else w, True))
    return steps


def head(case, dtype=torch.float64):
    """(d_rgb [P,64], d_sig [P]) in `dtype`"""
    out, d = case["out"].to(dtype), case["d_out"].to(dtype)
    f = out[:, :FEAT]
    return d[:, :FEAT] * f * (1 - f), d[:, FEAT] * (1 - torch.exp(-out[:, FEAT]))


def reference(case):
    """{"d_rgb" [P,64], "d_sig" [P], "deltas": ten float64 tensors [P,256] (slot 9: [P,128])}: the explicit chain of the module docstring"""
    d_rgb, d_sig = head(case)
    deltas, cur = [None] * SLOTS, d_rgb
    for slot, w, masked in chain_steps(case):
        cur = cur @ w.double()
        if slot == 7:
            cur = cur + d_sig[:, None] * _w(case, "static_sigma.0").double()
        if masked:
            cur = cur * bits_to_mask(case["bits"][slot])[:, :cur.shape[1]]
        deltas[slot] = cur
    return {"d_rgb": d_rgb, "d_sig": d_sig, "deltas": deltas}


def expected32(ref):
    """The reference as the fp32 tensors a kernel must return -- after checking that the rounding changes nothing."""
    out = {}
    for k in ("d_rgb", "d_sig"):
        out[k] = ref[k].float()
        assert torch.equal(out[k].double(), ref[k]), k + ": the expected value is no fp32 number"
    out["deltas"] = [d.float() for d in ref["deltas"]]
    for s, (a, b) in enumerate(zip(out["deltas"], ref["deltas"])):
        assert torch.equal(a.double(), b), "slot %d: the expected value is no fp32 number" % s
    return out


def quantum(t):
    """The largest power of two that divides every entry of a tensor of dyadic numbers (inf for an all-zero one)."""
    v = t.detach().double().abs().flatten()
    v = v[v != 0]
    if v.numel() == 0:
        return math.inf
    mant, exp = torch.frexp(v)
    n = (mant * 2.0 ** 53).long()
    return float(((n & -n).double() * torch.exp2((exp - 53).double())).min())


def certificate(case):
    """Asserts for every sum of the chain, per point and column, sum |terms| * SPLIT_SLACK < 2^24 q (q: the product of the two operands' quanta, the
    smaller of the two for slot 7, which adds the sigma head), that the sigmoid' and softplus' factors are exact, and that reference(case) equals its
    own fp32 rounding.  Returns {slot: log2 of the worst sum / q}, all below 24 (slot 10: d_rgb, 11: d_sig -- single products)."""
    ref = reference(case)
    expected32(ref)
    d32 = head(case, torch.float32)
    assert torch.equal(d32[0].double(), ref["d_rgb"]) and torch.equal(d32[1].double(), ref["d_sig"]), "an fp32 head differs from float64"
    sp = 1 - torch.exp(-case["out"][:, FEAT].double())
    assert bool(((sp == 0) | (sp == 1)).all()), "softplus' is neither 0 nor 1"
    bits = {10: math.log2(max(float(ref["d_rgb"].abs().max()) / quantum(ref["d_rgb"]), 1.0)), 11: 0.0}
    cur = ref["d_rgb"]
    for slot, w, masked in chain_steps(case):
        q = quantum(cur) * quantum(w)
        s = cur.abs() @ w.double().abs()
        if slot == 7:
            ws = _w(case, "static_sigma.0").double()
            s = s + ref["d_sig"].abs()[:, None] * ws.abs()
            q = min(q, quantum(ref["d_sig"]) * quantum(ws))
        worst = float(s.max()) * SPLIT_SLACK / q if q != math.inf else 0.0
        bits[slot] = math.log2(worst) if worst > 0 else -math.inf
        assert bits[slot] < 24.0, "%s P=%d: slot %d needs %.2f bits" % (case["family"], case["P"], slot, bits[slot])
        cur = ref["deltas"][slot]
    return bits


def closed_form_bits(weights, gmax):
    """The same bound from the weights alone, for ANY number of points with |d_out| <= gmax: magnitudes through the largest column sums, quanta
    through the weights' quanta, from d_rgb's 1/16.  {slot: bits}."""
    case = {"weights": weights}
    mag, q, bits = gmax / 4.0, 1.0 / 16.0, {}
    for slot, w, masked in chain_steps(case):
        mag, q = mag * float(w.double().abs().sum(0).max()), q * quantum(w)
        if slot == 7:
            ws = _w(case, "static_sigma.0").double()
            mag, q = mag + gmax * float(ws.abs().max()), min(q, quantum(ws))
        bits[slot] = math.log2(mag * SPLIT_SLACK / q)
    return bits


def wgrad_certificate(wcase):
    """tests/_wgrad_cases.py's certificate for a case whose deltas are dyadic, not integers: sum_p |D| |A| < 2^24 q_d q_a per weight entry,
    sum_p |D| < 2^24 q_d per bias entry, and the float64 gradients equal their fp32 rounding.  {job: bits}"""
    bits = {}
    for name, D, blocks in _WG.jobs(wcase):
        Dabs, qd = D.double().abs(), quantum(D)
        worst = float(Dabs.sum(0).max()) / qd if qd != math.inf else 0.0
        for A in blocks:
            qa = quantum(A)
            if qd != math.inf and qa != math.inf:
                worst = max(worst, float((Dabs.T @ A.double().abs()).max()) / (qd * qa))
        bits[name] = math.log2(worst) if worst > 0 else -math.inf
        assert bits[name] < 24.0, "P=%d: %s needs %.2f bits" % (wcase["P"], name, bits[name])
    for name, r in zip(TENSOR_NAMES, _WG.reference(wcase)):
        assert torch.equal(r.float().double(), r), name + ": the expected value is no fp32 number"
    return bits


# ------------------------------------------------------------------------------------------------------------------ which cores are fair
def point_scale(d):
    """point_scale_h (csrc/mlp_backward_h2.hip): 2^(134 - e) per point, e = the exponent field of the row's largest |delta|, clamped to [32, 254]"""
    m = d.double().abs().amax(1)
    _, ex = torch.frexp(m.float())
    e = torch.where(m > 0, ex + 126, torch.zeros_like(ex)).clamp(32, 254)
    return torch.exp2((134 - e).double())[:, None]


def pieces_f16(s):
    """The two-piece fp16 split of float64 values (h2_split_first / _second, csrc/mlp_core_h2.h): h1 = fp16(s), h2 = fp16(s - h1).  -> (h2, whether
    h1 + h2 == s with every piece finite and no non-zero piece an fp16 subnormal)"""
    h1 = s.to(torch.float16).double()
    h2 = (s - h1).to(torch.float16).double()
    sub = any(bool(((h != 0) & (h.abs() < 2.0 ** -14)).any()) for h in (h1, h2))
    return h2, bool(torch.isfinite(h1).all()) and bool((h1 + h2 == s).all()) and not sub


def fair_cores(case, ref=None):
    """The cores whose piece products lose nothing on this case.  fp32: always (the certificate is the condition).  h2: every row that a layer
    walks, scaled per point, and every weight times 2^8 splits exactly into two fp16 pieces, and the dropped product (second piece x second piece)
    is zero.  x3: three bf16 pieces each (round to nearest, csrc/mlp_core_x3.h: x3_split); the dropped products are 2 x 3, 3 x 2, 3 x 3."""
    ref = ref or reference(case)
    ok = {c: True for c in CORES}
    src = ref["d_rgb"]
    for slot, w, masked in chain_steps(case):
        ok["h2"] &= float(w.abs().max()) < 255.0
        d2, dex = pieces_f16(src * point_scale(src))
        w2, wex = pieces_f16(w.double() * 256.0)
        ok["h2"] &= dex and wex and not (bool(d2.any()) and bool(w2.any()))
        pd, pex = pieces_bf16(src.float())
        pw, wex3 = pieces_bf16(w.float())
        nd, nw = 1 + int(bool(pd[1].any())) + int(bool(pd[2].any())), 1 + int(bool(pw[1].any())) + int(bool(pw[2].any()))
        ok["x3"] &= pex and wex3 and not (nd >= 3 and nw >= 2) and not (nw >= 3 and nd >= 2)
        src = ref["deltas"][slot]
    return tuple(c for c in CORES if ok[c])


def pieces_used(ref):
    """(most bf16 pieces, most fp16 pieces) that a row walked by a layer needs: what a family reaches"""
    nb = nh = 1
    for src in [ref["d_rgb"]] + [ref["deltas"][s] for s in range(9, 0, -1)]:
        p, _ = pieces_bf16(src.float())
        nb = max(nb, 1 + int(bool(p[1].any())) + int(bool(p[2].any())))
        nh = max(nh, 1 + int(bool(pieces_f16(src * point_scale(src))[0].any())))
    return nb, nh


def range_words(ref):
    """The eleven words an h2 data gradient leaves for the f16x2 weight gradients: the bits of max |delta| per slot (slot 9: its 128 columns), then d_rgb's"""
    return [range_word(d) for d in ref["deltas"]] + [range_word(ref["d_rgb"])]


# ------------------------------------------------------------------------------------------------------------------ fp32 in two orders
def chain_fp32(case, order="plain"):
    """The chain in fp32 numpy, the sums taken term by term in one of two orders: "plain" (rows ascending) or "reversed-chunked" (rows descending,
    four partial sums of every fourth row, then added).  -> like reference(), fp32"""
    f32 = np.float32
    d_rgb, d_sig = (t.numpy() for t in head(to_device(case, "cpu"), torch.float32))
    deltas, cur = [None] * SLOTS, d_rgb
    for slot, w, masked in chain_steps(to_device(case, "cpu")):
        w = w.numpy().astype(f32)
        rows = np.arange(w.shape[0]) if order == "plain" else np.arange(w.shape[0])[::-1]
        lanes = 1 if order == "plain" else 4
        part = np.zeros((lanes, cur.shape[0], w.shape[1]), dtype=f32)
        for n, r in enumerate(rows):
            if w[r].any():
                part[n % lanes] += cur[:, r:r + 1] * w[r][None, :]
        acc = part[0] if lanes == 1 else (part[0] + part[1]) + (part[2] + part[3])
        if slot == 7:
            ws = _w(case, "static_sigma.0").cpu().numpy().astype(f32)
            acc = acc + d_sig[:, None] * ws if order == "plain" else d_sig[:, None] * ws + acc
        if masked:
            acc = np.where(bits_to_mask(case["bits"][slot].cpu())[:, :acc.shape[1]].numpy(), acc, f32(0))
        assert acc.dtype == f32
        deltas[slot] = cur = acc
    return {"d_rgb": d_rgb, "d_sig": d_sig, "deltas": deltas}


# ------------------------------------------------------------------------------------------------------------------ the kernels' index arithmetic
MUTANTS = ("word g+1", "bit 4t+r with the split cores' tile", "slot 8 masked", "sigma head dropped", "offset 92", "dir columns first", "slots 2 and 3 swapped")


def _lane_map(lanes):
    """Per feature 0..255: (the mask word, the bit) that the lane holding it tests.  "g4": mlp_backward16_kernel -- lane group g = lane >> 4 holds
    registers dl[T][r] = feature 16 T + 4 g + r and tests bit 4 T + r of word g (finish_delta).  "h2": the split cores -- lane half h = lane >> 5 holds
    dl[t][4 q + j] = feature 32 t + 8 q + 4 h + j and tests bit 4 (2 t + (q >> 1)) + j of word h + 2 (q & 1) (finish_delta_h, finish_delta_x)."""
    word, bit = np.full(W, -1), np.full(W, -1)
    if lanes == "g4":
        for g in range(4):
            for T in range(16):
                for r in range(4):
                    word[16 * T + 4 * g + r], bit[16 * T + 4 * g + r] = g, 4 * T + r
    else:
        for h in range(2):
            for t in range(8):
                for q in range(4):
                    for j in range(4):
                        word[32 * t + 8 * q + 4 * h + j], bit[32 * t + 8 * q + 4 * h + j] = h + 2 * (q & 1), 4 * (2 * t + (q >> 1)) + j
    assert (word >= 0).all() and (bit >= 0).all()
    return word, bit


def emulate(case, lanes, mutant=None):
    """The data gradient as the kernels index it (float64 numpy; the arithmetic is not the point here): slot order, the two lane layouts' mask bits,
    the skip's offset 93, dir_encoding's 256-column cut, slot 9's 128 columns, the sigma head.  mutant: one of MUTANTS, a one-line slip each."""
    assert mutant is None or mutant in MUTANTS
    case = to_device(case, "cpu")
    word, bit = _lane_map(lanes)
    if mutant == "word g+1":
        word = (word + 1) & 3
    if mutant == "bit 4t+r with the split cores' tile":                  # t = feature >> 5 where T = 2 t + (q >> 1) = feature >> 4 belongs
        bit = 4 * (np.arange(W) >> 5) + (np.arange(W) & 3)
    words = case["bits"].numpy().astype(np.uint64)                       # [10, P, 4]
    relu = lambda slot, n: ((words[slot][:, word[:n]] >> bit[:n].astype(np.uint64)) & np.uint64(1)).astype(bool)   # noqa: E731
    wt = {n: t.double().numpy() for n, t in zip(TENSOR_NAMES, case["weights"])}
    d_rgb, d_sig = (t.numpy() for t in head(case))
    deltas = [None] * SLOTS
    d9 = np.where(relu(9, 128), d_rgb @ wt["static_rgb.0.weight"], 0.0)
    deltas[9] = d9
    d8 = d9 @ (wt["dir_encoding.0.weight"][:, DIR:DIR + W] if mutant == "dir columns first" else wt["dir_encoding.0.weight"][:, :W])
    if mutant == "slot 8 masked":
        d8 = np.where(relu(8, W), d8, 0.0)
    deltas[8] = d8
    acc = d8 @ wt["xyz_encoding_final.weight"]
    if mutant != "sigma head dropped":
        acc = acc + d_sig[:, None] * wt["static_sigma.0.weight"]
    cur = deltas[7] = np.where(relu(7, W), acc, 0.0)
    for l in range(7, 0, -1):
        w = wt["xyz_encoding_%d.0.weight" % (l + 1)]
        if l + 1 == 5:
            w = w[:, (92 if mutant == "offset 92" else XYZ):][:, :W]
        tgt = l - 1
        if mutant == "slots 2 and 3 swapped" and tgt in (2, 3):
            tgt = 5 - tgt
        cur = np.where(relu(tgt, W), cur @ w, 0.0)
        deltas[l - 1] = cur
    return {"d_rgb": d_rgb, "d_sig": d_sig, "deltas": deltas}


def same(a, ref):
    """Does an emulation / fp32 evaluation (numpy) equal the reference (torch float64) bit for bit?"""
    pairs = [(a["d_rgb"], ref["d_rgb"]), (a["d_sig"], ref["d_sig"])] + list(zip(a["deltas"], ref["deltas"]))
    return all(np.array_equal(np.asarray(x, dtype=np.float64), y.cpu().numpy()) for x, y in pairs)


# ------------------------------------------------------------------------------------------------------------------ the forward twin
# ops.mlp_forward_train leaves all ten activation rows and the relu words in the saved state.  With integer x, weights +-1 (k per column as below,
# the sigma head 16 entries) and integer biases every pre-activation is a small integer: the rows are exact in any summation order, and the
# pre-activations tie at 0 all the time, so the relu words pin the rule `> 0`.  The heads' biases are set so that x = 0 gives pre-activation 0, and a
# point whose head pre-activations leave [-PRE_BOUND, PRE_BOUND] gets x = 0 instead (about one in fifty): `out` (sigmoid / softplus, not exact) is then compared where one
# quantum of the pre-activation moves it by 1.5e-3 or more.  sigma_shift = SIGMA_HIGH moves the sigma pre-activations to 18..30, around softplus's threshold 20.
FWD_K = {"xyz_encoding_1.0": 3, "xyz_encoding_3.0": 2, "xyz_encoding_5.0": 2, "xyz_encoding_7.0": 2, "xyz_encoding_final": 2, "dir_encoding.0": 2}
PRE_BOUND, SIGMA_HIGH = 6.0, 24.0


def forward(weights, x, dtype=torch.float64, pres=None):
    """NeRF_sigma.forward (models/nerf.py) spelled out: (the ten saved rows [slot 9: 128 columns], rgb pre-activation [P,64], sigma pre-activation [P]);
    pres: a list that receives the nine pre-activations that meet a relu"""
    w = {n: t.to(dtype) for n, t in zip(TENSOR_NAMES, weights)}
    lin = lambda h, name: h @ w[name + ".weight"].T + w[name + ".bias"]          # noqa: E731
    x = x.to(dtype)
    xyz, dirs = x[:, :XYZ], x[:, XYZ:]
    h, acts = xyz, []
    for l in range(1, 9):
        pre = lin(torch.cat([xyz, h], 1) if l == 5 else h, "xyz_encoding_%d.0" % l)
        h = torch.relu(pre)
        acts.append(h)
        if pres is not None:
            pres.append(pre)
    final = lin(h, "xyz_encoding_final")
    pre = lin(torch.cat([final, dirs], 1), "dir_encoding.0")
    g = torch.relu(pre)
    if pres is not None:
        pres.append(pre)
    return acts + [final, g], lin(g, "static_rgb.0"), lin(h, "static_sigma.0")[:, 0]


def make_forward_weights(seed, sigma_shift=0.0):
    gen = torch.Generator()
    gen.manual_seed(seed * 104729 + 1)
    out = []
    for name, (n_out, n_in) in zip(LAYERS, SHAPES[0::2]):
        if name == "static_sigma.0":
            w = torch.zeros(1, n_in)
            w[0, torch.randperm(n_in, generator=gen)[:16]] = (torch.randint(0, 2, (16,), generator=gen) * 2 - 1).float()
        else:
            w = _sparse(n_out, n_in, FWD_K.get(name, 1), (1.0,), gen)
        out += [w, torch.randint(-1, 2, (n_out,), generator=gen).float()]
    _, rgb0, sig0 = forward(out, torch.zeros(1, XYZ + DIR))
    out[TENSOR_NAMES.index("static_rgb.0.bias")] -= rgb0[0].float()
    out[TENSOR_NAMES.index("static_sigma.0.bias")] += sigma_shift - float(sig0[0])
    return out


def make_forward_case(P, seed, device="cpu", sigma_shift=0.0):
    """{"P", "weights", "x" [P,120] integers -2..2 (half zero), "sigma_shift"} on `device`"""
    gen = torch.Generator(device=device)
    gen.manual_seed(seed * 1000003 + P + 17)
    ri = lambda lo, hi: torch.randint(lo, hi, (P, XYZ + DIR), generator=gen, device=device, dtype=torch.int64)   # noqa: E731
    x = (ri(1, 3) * ri(0, 2) * (ri(0, 2) * 2 - 1)).float()
    weights = [w.to(device) for w in make_forward_weights(seed, sigma_shift)]
    _, rgb, sig = forward(weights, x)
    x[(rgb.abs().amax(1) > PRE_BOUND) | ((sig - sigma_shift).abs() > PRE_BOUND)] = 0.0
    return {"P": P, "weights": weights, "x": x, "sigma_shift": sigma_shift}


def forward_reference(case):
    """{"acts" (ten float64 rows), "bits" [10,P,4] (`> 0`; slot 8 zero), "pre_rgb", "pre_sig", "out" [P,65] = float64 sigmoid / softplus}"""
    acts, rgb, sig = forward(case["weights"], case["x"])
    bits = torch.stack([mask_to_bits(a > 0) if s != 8 else torch.zeros(case["P"], 4, dtype=torch.int64, device=a.device) for s, a in enumerate(acts)])
    out = torch.cat([torch.sigmoid(rgb), torch.nn.functional.softplus(sig)[:, None]], 1)
    return {"acts": acts, "bits": bits, "pre_rgb": rgb, "pre_sig": sig, "out": out}


def forward_certificate(case, ref=None):
    """The certificate for the forward sums: per point and output feature sum |x_i w_i| + |b| < 2^24 q, every row its own fp32 rounding, the heads'
    pre-activations inside the bound.  {layer: bits}"""
    ref = ref or forward_reference(case)
    w = dict(zip(TENSOR_NAMES, case["weights"]))
    x = case["x"].double()
    acts = ref["acts"]
    ins = [x[:, :XYZ]] + acts[0:3] + [torch.cat([x[:, :XYZ], acts[3]], 1)] + acts[4:7] + [acts[7], acts[7], torch.cat([acts[8], x[:, XYZ:]], 1), acts[9]]
    bits = {}
    for name, a in zip(LAYERS, ins):
        wt, b = w[name + ".weight"].double(), w[name + ".bias"].double()
        q = min(quantum(a) * quantum(wt), quantum(b))
        s = float((a.abs() @ wt.abs().T + b.abs()).max())
        bits[name] = math.log2(max(s / q, 1.0)) if q != math.inf else 0.0
        assert bits[name] < 24.0, "forward P=%d: %s needs %.2f bits" % (case["P"], name, bits[name])
    for s, a in enumerate(acts):
        assert torch.equal(a.float().double(), a), "forward slot %d: the expected value is no fp32 number" % s
    assert float(ref["pre_rgb"].abs().max()) <= PRE_BOUND and float((ref["pre_sig"] - case["sigma_shift"]).abs().max()) <= PRE_BOUND
    assert quantum(ref["pre_rgb"]) >= 1.0 and quantum(ref["pre_sig"]) >= 1.0          # integers: one quantum of a pre-activation is 1
    return bits


def out_bar(oracle_forward, seed):
    """(the bar for `out`, the oracle's error behind it): four times the largest error of the fp32 CPU oracle (oracle_forward(state, x) -> [P,65])
    against float64 on the forward cases -- every head pre-activation is one of the few integers in [-PRE_BOUND, PRE_BOUND] (sigma: also shifted by
    SIGMA_HIGH), so 2,049 points of either kind hold them all --, and never looser than the 1e-6 of the golden MLP test"""
    err = 0.0
    for shift in (0.0, SIGMA_HIGH):
        case = make_forward_case(2049, seed, sigma_shift=shift)
        got = oracle_forward(dict(zip(TENSOR_NAMES, case["weights"])), case["x"])
        assert got.dtype == torch.float32
        err = max(err, float((got.double() - forward_reference(case)["out"]).abs().max()))
    return min(1e-6, 4.0 * err), err

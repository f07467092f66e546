"""Exactly summable operands for the MLP weight gradients (csrc/mlp_train16.hip: wgrad_body<0|1|2|4>, wgrad_batch, the two reduce kernels,
launch_mlp_wgrads and its chunk planning), their float64 reference, the certificate that makes "bit for bit" a fair demand, and the byte layout
of the saved state and the backward's scratch buffer.  Shared by tests/test_wgrad_exact_host.py (CPU) and tests/test_gpu_wgrad_exact.py; imports
numpy and torch only -- never the product package.

THE IDEA.  dW[m][n] = sum_p D[p][m] * A[p][n] has no non-linearity.  If every delta is a multiple of one power of two q_d, every input a multiple of
q_a, and sum_p |D[p][m]| |A[p][n]| < 2^24 q_d q_a for every (m, n) (and sum_p |D[p][m]| < 2^24 q_d for the bias sums), then every partial sum in ANY
order is an fp32 number: chunked or not, reduced in any tree, on the fp32 MFMA or as bf16 / fp16 piece products, a kernel that forms the right terms
gives the float64 result to the bit -- and one that drops, doubles or misplaces a single point does not.  No tolerance is involved.

THE SPLIT MODES take part as long as each operand's pieces are exact (fair_modes() checks it on the data, by emulating the splits):
  bf16     single piece: every operand is a bf16 number (at most 8 significant bits)
  bf16x3   three RNE pieces hold up to 24 bits; the piece products d2 a3, d3 a2, d3 a3 are dropped, so an operand with a third piece may only meet
           single-piece operands
  f16x2    two pieces (scaled by the power of two that the range word gives) hold up to 22 bits; d2 a2 is dropped, so at most one operand of a pair
           has a second piece; and no piece may be an fp16 subnormal -- guaranteed when all of a tensor's non-zero values lie within 2^6 of
           its largest, which is how the wide families are drawn

THE FAMILIES (FAMILIES below).  An operand is drawn from integers of magnitude <= m, about half of them zero:
  narrow          deltas -2..2, inputs 0..15: certified for every P up to 2^18 + 1, since 2 * 15 * (2^18 + 1) < 2^24
  narrow_signed   the same with inputs -15..15
  wide_1_17       deltas -1..1, inputs of 17 bits (second bf16 and fp16 pieces in the INPUT operand), P <= 64
  wide_17_1       the mirror image, P <= 64
  wide_1_18       deltas -1..1, inputs of 18 bits, P <= 32: THIRD bf16 pieces.  (A round-to-nearest split is signed: the remainder of a 17-bit integer
                  behind its first 8-bit piece is at most 2^8 in magnitude and fits the second piece, so 17 bits never reach a third one -- checked in
                  tests/test_wgrad_exact_host.py.)
  wide_18_1       the mirror image, P <= 32
  wide_6_11       deltas of 6 bits, inputs of 11, P <= 128
EDGE CONTENTS, so that an index slip shows: the last point of the case is non-zero in every column of every operand (so every column is non-zero
somewhere, at P = 1 too), and it and the last point of each 128-point block carry magnitudes that no other point has in those columns (m and
m - 1, resp. m - 2 and m - 3; with m = 2: +-2 against -1..1 elsewhere, the two kinds with opposite signs; with m = 1 only the sign pattern is
left).  The marks alternate with the column, so each column differs from its neighbours already at P = 1 -- the last column of every job (92, 26,
127, 63, 255) and the first one past it.  The columns a job does NOT use (128..255 of activation slot 9 and of delta slot 9) are filled like the
others: a kernel that reads them shows up, the reference ignores them.
"""
import math

import numpy as np
import torch

MODES = ("fp32", "bf16", "bf16x3", "f16x2")
XYZ, DIR, IN_DIM, W, SLOTS, FEAT = 93, 27, 120, 256, 10, 64
RANGE_WORDS, RANGE_USED, ACTS_RANGE_BYTES = 64, 11, 256
TENSOR_NAMES = ([n for i in range(1, 9) for n in ("xyz_encoding_%d.0.weight" % i, "xyz_encoding_%d.0.bias" % i)]
                + ["xyz_encoding_final.weight", "xyz_encoding_final.bias", "static_sigma.0.weight", "static_sigma.0.bias",
                   "dir_encoding.0.weight", "dir_encoding.0.bias", "static_rgb.0.weight", "static_rgb.0.bias"])

# md, ma: largest magnitude of a delta / an input; signed_a: inputs of both signs; modes: the modes the family is fair for; max_P: certified up to there
FAMILIES = {
    "narrow": dict(md=2, ma=15, signed_a=False, modes=MODES, max_P=2 ** 18 + 1),
    "narrow_signed": dict(md=2, ma=15, signed_a=True, modes=MODES, max_P=2 ** 18 + 1),
    "wide_1_17": dict(md=1, ma=2 ** 17 - 1, signed_a=True, modes=("fp32", "bf16x3", "f16x2"), max_P=64),
    "wide_17_1": dict(md=2 ** 17 - 1, ma=1, signed_a=True, modes=("fp32", "bf16x3", "f16x2"), max_P=64),
    "wide_1_18": dict(md=1, ma=2 ** 18 - 1, signed_a=True, modes=("fp32", "bf16x3", "f16x2"), max_P=32),
    "wide_18_1": dict(md=2 ** 18 - 1, ma=1, signed_a=True, modes=("fp32", "bf16x3", "f16x2"), max_P=32),
    "wide_6_11": dict(md=2 ** 6 - 1, ma=2 ** 11 - 1, signed_a=True, modes=("fp32", "bf16x3", "f16x2"), max_P=128),
}


def closed_form_bits(P, md, ma):
    """log2 of the largest sum of |terms| that operands of magnitude <= md, ma can form over P points (quanta 1): the certificate of a case too
    large to build on the CPU.  Below 24 = certified."""
    return math.log2(max(md * ma, md) * P)


def _operand(P, ncols, m, signed, gen, device):
    """[P, ncols] fp32: integers of magnitude <= m, half of them zero, with the edge marks of the module docstring."""
    lo, hi = (1, 1) if m <= 2 else (max(1, (m + 1) >> 6), m - 4)
    mag = torch.randint(lo, hi + 1, (P, ncols), generator=gen, device=device, dtype=torch.int32)
    mag *= torch.randint(0, 2, (P, ncols), generator=gen, device=device, dtype=torch.int32)
    if signed:
        mag *= torch.randint(0, 2, (P, ncols), generator=gen, device=device, dtype=torch.int32) * 2 - 1
    c = torch.arange(ncols, device=device, dtype=torch.int32)
    if m <= 2:
        assert signed
        last, block = m * (1 - 2 * (c & 1)), -m * (1 - 2 * (c & 1))
    else:
        sgn = 1 - 2 * ((c >> 1) & 1) if signed else torch.ones_like(c)
        last, block = (m - 1 + (c & 1)) * sgn, (m - 3 + (c & 1)) * sgn
    mag[127::128] = block
    mag[P - 1] = last
    return mag.to(torch.float32)


def make_case(P, family, seed, device="cpu"):
    """{"P", "family", "x" [P,120], "acts" 10 x [P,256], "deltas" 10 x [P,256], "d_rgb" [P,64], "d_sig" [P]}: fp32 tensors on `device` (the random
    streams of two devices differ; a case is certified by certificate(), or by closed_form_bits() where it is too large for that)."""
    f = FAMILIES[family]
    assert 1 <= P <= f["max_P"], (P, family)
    gen = torch.Generator(device=device)
    gen.manual_seed(seed * 1000003 + P)
    A = lambda n: _operand(P, n, f["ma"], f["signed_a"], gen, device)   # noqa: E731
    D = lambda n: _operand(P, n, f["md"], True, gen, device)            # noqa: E731
    return {"P": P, "family": family, "x": A(IN_DIM), "acts": [A(W) for _ in range(SLOTS)], "deltas": [D(W) for _ in range(SLOTS)],
            "d_rgb": D(FEAT), "d_sig": D(1)[:, 0].contiguous()}


# ------------------------------------------------------------------------------------------------------------------ reference
def jobs(case):
    """The eleven nn.Linear of NeRF_sigma (models/nerf.py) as (name, delta [P,M], [input blocks]): which saved tensor is each layer's input, which
    delta its output gradient.  acts = h1..h8, xyz_encoding_final's output, dir_encoding's output; deltas = the gradients at the outputs of
    xyz_encoding_1..8, xyz_encoding_final, dir_encoding.  xyz_encoding_5 reads cat([xyz, h4]), dir_encoding reads cat([final, dir])."""
    x, a, d = case["x"], case["acts"], case["deltas"]
    xyz, dirs = x[:, :XYZ], x[:, XYZ:]
    out = [("xyz_encoding_1.0", d[0], [xyz])]
    for i in range(2, 9):
        out.append(("xyz_encoding_%d.0" % i, d[i - 1], [xyz, a[i - 2]] if i == 5 else [a[i - 2]]))
    out.append(("xyz_encoding_final", d[8], [a[7]]))
    out.append(("static_sigma.0", case["d_sig"][:, None], [a[7]]))
    out.append(("dir_encoding.0", d[9][:, :128], [a[8], dirs]))
    out.append(("static_rgb.0", case["d_rgb"], [a[9][:, :128]]))
    return out


def reference(case):
    """The 24 gradients in TENSOR_NAMES order (= ops.MLP_TENSOR_NAMES), float64: D.T @ A per job, column sums of D for the bias."""
    out = []
    for name, D, blocks in jobs(case):
        D64 = D.double()
        out += [torch.cat([D64.T @ A.double() for A in blocks], 1), D64.sum(0)]
    return out


def quantum(t):
    """The largest power of two that divides every entry of an integer-valued tensor (inf for an all-zero one)."""
    v = t.detach().double().abs().flatten()
    v = v[v != 0]
    if v.numel() == 0:
        return math.inf
    assert bool((v == v.round()).all()) and float(v.max()) < 2.0 ** 53, "the cases hold integers"
    n = v.long()
    return float((n & -n).min())


def certificate(case):
    """Asserts, per job and in float64, sum_p |D| |A| < 2^24 q_d q_a for every weight entry and sum_p |D| < 2^24 q_d for every bias entry (q: the
    operand's quantum), and that reference(case) equals its own fp32 rounding.  Returns {job: log2 of the worst sum / quantum}, all below 24."""
    bits = {}
    for name, D, blocks in jobs(case):
        Dabs, qd = D.double().abs(), quantum(D)
        worst = float(Dabs.sum(0).max()) / qd if qd != math.inf else 0.0
        for A in blocks:
            qa = quantum(A)
            if qd != math.inf and qa != math.inf:
                worst = max(worst, float((Dabs.T @ A.double().abs()).max()) / (qd * qa))
        bits[name] = math.log2(worst) if worst > 0 else -math.inf
        assert bits[name] < 24.0, "%s P=%d: %s needs %.2f bits" % (case["family"], case["P"], name, bits[name])
    for name, r in zip(TENSOR_NAMES, reference(case)):
        assert torch.equal(r.float().double(), r), name + ": the expected value is no fp32 number"
    return bits


# ------------------------------------------------------------------------------------------------------------------ piece rules
def _bits_of(v):
    return v.contiguous().view(torch.int32)


def range_word(t):
    """The bits of max |t| as an int: what the h2 data gradient leaves in a delta slot's range word, and the h2 forward in the saved state's."""
    return int(_bits_of(t.detach().abs().max().float().reshape(1).cpu())[0])


def true_words(case):
    """(the 11 delta range words: slots 0..9 and d_rgb, true maxima; the activation word: the true maximum of x and the activation rows)"""
    return [range_word(d) for d in case["deltas"]] + [range_word(case["d_rgb"])], max([range_word(case["x"])] + [range_word(a) for a in case["acts"]])


def pieces_bf16(v):
    """wgrad's three-piece split (RNE): [w1, w2, w3] as fp32 tensors and whether w1 + w2 + w3 == v exactly"""
    w1 = v.to(torch.bfloat16).float()
    w2 = (v - w1).to(torch.bfloat16).float()
    w3 = (v - w1 - w2).to(torch.bfloat16).float()
    return [w1, w2, w3], bool((w1.double() + w2.double() + w3.double() == v.double()).all())


def delta_scale(word):
    """delta_scale_h: 2^(140 - e) with e the word's exponent field clamped to [32, 254]"""
    return 2.0 ** (140 - min(max((word >> 23) & 0xff, 32), 254))


def act_scale(word):
    """act_scale_h: 1 for an exponent field of 0 or 255, else 2^(141 - e) with e clamped to [103, 165]"""
    e = (word >> 23) & 0xff
    return 1.0 if e in (0, 255) else 2.0 ** (141 - min(max(e, 103), 165))


def pieces_f16(v, scale):
    """wgrad's two-piece fp16 split of v * scale: [h1, h2], whether h1 + h2 == v * scale exactly with every piece finite, and whether some non-zero
    piece is an fp16 subnormal"""
    s = v.double() * scale
    h1 = s.to(torch.float16).double()
    h2 = (s - h1).to(torch.float16).double()
    exact = bool(torch.isfinite(h1).all()) and bool((h1 + h2 == s).all())
    return [h1, h2], exact, any(bool(((h != 0) & (h.abs() < 2.0 ** -14)).any()) for h in (h1, h2))


def fair_modes(case):
    """The modes in which EVERY job of the case has exact pieces and loses none of its piece products (the rules of the module docstring, decided by
    splitting the data itself; f16x2 with the true range words).  static_sigma always runs on the fp32 MFMA."""
    dwords, aword = true_words(case)
    slot_word = {id(d): w for d, w in zip(case["deltas"] + [case["d_rgb"]], dwords)}
    ok = {m: True for m in MODES}
    for name, D, blocks in jobs(case):
        if name == "static_sigma.0":
            continue
        word = dwords[9] if name == "dir_encoding.0" else slot_word[id(D)]
        pd, exact_d = pieces_bf16(D)
        (_, d2), hexact_d, dsub = pieces_f16(D, delta_scale(word))
        for A in blocks:
            pa, exact_a = pieces_bf16(A)
            (_, a2), hexact_a, asub = pieces_f16(A, act_scale(aword))
            ok["bf16"] &= not bool(pd[1].any()) and not bool(pa[1].any())
            nd, na = 1 + int(bool(pd[1].any())) + int(bool(pd[2].any())), 1 + int(bool(pa[1].any())) + int(bool(pa[2].any()))
            ok["bf16x3"] &= exact_d and exact_a and not (nd >= 3 and na >= 2) and not (na >= 3 and nd >= 2)
            ok["f16x2"] &= hexact_d and hexact_a and not dsub and not asub and not (bool(d2.any()) and bool(a2.any()))
    return tuple(m for m in MODES if ok[m])


# ------------------------------------------------------------------------------------------------------------------ byte layout
def _f32(buf, byte0, n):
    return buf[byte0:byte0 + 4 * n].view(torch.float32)


def _i32(buf, byte0, n):
    return buf[byte0:byte0 + 4 * n].view(torch.int32)


def layout(P):
    """Byte offsets.  Saved state (csrc/mlp_train16.h, csrc/kernels.h): acts[10][P][256] fp32 | relu bits [10][P] x 32 B | the range word's 256-byte
    line.  Scratch (launch_mlp_backward, mlp_train_scratch_bytes): deltas[10][P][256] fp32 | d_rgb[P][64] | d_sig[P] | 64 range words | workspace."""
    rows = SLOTS * P * W * 4
    return {"masks": rows, "amax": rows + SLOTS * P * 32, "acts_min": rows + SLOTS * P * 32 + ACTS_RANGE_BYTES,
            "d_rgb": rows, "d_sig": rows + P * FEAT * 4, "dmax": rows + P * FEAT * 4 + P * 4, "ws": rows + P * FEAT * 4 + P * 4 + RANGE_WORDS * 4}


def pack_state(case, acts_bytes, scratch_bytes, dmax_words=None, amax_word=0):
    """-> (acts buffer, scratch buffer): zero-filled uint8 tensors of the given sizes on the case's device, holding the case in the product's layout.
    The relu bits stay zero (the weight gradients do not read them); dmax_words: up to 64 ints (bit patterns), missing ones zero."""
    P, L, dev = case["P"], layout(case["P"]), case["x"].device
    assert acts_bytes >= L["acts_min"] and scratch_bytes >= L["ws"], (acts_bytes, scratch_bytes, L)
    acts = torch.zeros(acts_bytes, dtype=torch.uint8, device=dev)
    scratch = torch.zeros(scratch_bytes, dtype=torch.uint8, device=dev)
    for s in range(SLOTS):
        _f32(acts, s * P * W * 4, P * W).view(P, W).copy_(case["acts"][s])
        _f32(scratch, s * P * W * 4, P * W).view(P, W).copy_(case["deltas"][s])
    _f32(scratch, L["d_rgb"], P * FEAT).view(P, FEAT).copy_(case["d_rgb"])
    _f32(scratch, L["d_sig"], P).copy_(case["d_sig"])
    words = list(dmax_words or [])
    assert len(words) <= RANGE_WORDS and all(-2 ** 31 <= w < 2 ** 31 for w in words + [amax_word])      # int32 bit patterns
    _i32(scratch, L["dmax"], RANGE_WORDS).copy_(torch.tensor(words + [0] * (RANGE_WORDS - len(words)), dtype=torch.int32))
    _i32(acts, L["amax"], 1).fill_(amax_word)
    return acts, scratch


def unpack_state(x, acts, scratch, P, family=None):
    """The inverse: a case (copies) plus "dmax_words" (64 ints) and "amax_word"."""
    L = layout(P)
    return {"P": P, "family": family, "x": x.clone(),
            "acts": [_f32(acts, s * P * W * 4, P * W).view(P, W).clone() for s in range(SLOTS)],
            "deltas": [_f32(scratch, s * P * W * 4, P * W).view(P, W).clone() for s in range(SLOTS)],
            "d_rgb": _f32(scratch, L["d_rgb"], P * FEAT).view(P, FEAT).clone(), "d_sig": _f32(scratch, L["d_sig"], P).clone(),
            "dmax_words": [int(w) for w in _i32(scratch, L["dmax"], RANGE_WORDS).cpu()], "amax_word": int(_i32(acts, L["amax"], 1).cpu()[0])}


def first_difference(got, want32):
    """None, or "k of n elements differ, first at index: got .., want .." (NaN counts as different)"""
    if got.shape == want32.shape and torch.equal(got, want32):
        return None
    if got.shape != want32.shape:
        return "shape %s, want %s" % (tuple(got.shape), tuple(want32.shape))
    bad = (got != want32) | got.isnan()
    idx = tuple(int(v) for v in bad.nonzero()[0])
    return "%d of %d elements differ, first at %s: got %r, want %r" % (int(bad.sum()), bad.numel(), idx, float(got[idx]), float(want32[idx]))


def numpy_chunked(D, A, order, chunk):
    """fp32 numpy: sum over chunks (in `order` of the points) of D[chunk].T @ A[chunk], accumulated in fp32 -- one of the many orders a kernel may use"""
    D, A = D.numpy().astype(np.float32)[order], A.numpy().astype(np.float32)[order]
    acc = np.zeros((D.shape[1], A.shape[1]), dtype=np.float32)
    for p0 in range(0, D.shape[0], chunk):
        acc = acc + D[p0:p0 + chunk].T @ A[p0:p0 + chunk]
    return acc

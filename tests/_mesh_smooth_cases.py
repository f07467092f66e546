"""The rules of csrc/crnerf_mesh_smooth.h restated in NumPy, and the hand cases of the smoothing tests (tests/test_mesh_smooth_host.py,
tests/test_gpu_mesh_smooth.py).  Test infrastructure: written from the rules, not from csrc/mesh_smooth.hip -- there is no neighbour list here:
the neighbour sums, the degrees and h are np.add.at over the corners of the faces into int64 and uint64; the pass, the output and the normal
formulas are spelled in float64 operation by operation, as the header states them (NumPy rounds every operation on its own).

adjacency_ref(faces, V) -> (d [V] int64, h [V] uint64)
smooth_ref(vertices, faces, lo, k, steps, lam, mu, pin_border=True) -> vertices' float32
normals_ref(vertices, faces, k2) -> normals float32
box_of(vertices) -> (lo, k, k2): what crnerf_amd.geometry.Mesh.smooth hands to the library"""
import math

import numpy as np

ONE = 2 ** 30


def valid_faces(faces, V):
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    return f[((f >= 0) & (f < V)).all(axis=1)]


def mix(ids):
    """The splitmix64 finaliser of the ids, wrapping in uint64."""
    with np.errstate(over="ignore"):
        z = np.asarray(ids).astype(np.uint64) + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def adjacency_ref(faces, V):
    """d_i = 2 x the valid incident faces; h_i = the sum of mix(next) - mix(prev) over them."""
    f = valid_faces(faces, V)
    d = np.zeros(V, np.int64)
    h = np.zeros(V, np.uint64)
    m = mix(f)
    with np.errstate(over="ignore"):
        for j in range(3):
            np.add.at(d, f[:, j], 2)
            np.add.at(h, f[:, j], m[:, (j + 1) % 3] - m[:, (j + 2) % 3])
    return d, h


def pinned_ref(faces, V, pin_border=True):
    d, h = adjacency_ref(faces, V)
    return (d == 0) | (h != 0) if pin_border else d == 0


def quantise_ref(vertices, lo, k):
    v = np.asarray(vertices, dtype=np.float32).reshape(-1, 3).astype(np.float64)
    lo = np.asarray(lo, dtype=np.float32).astype(np.float64)
    return np.clip(np.rint((v - lo) * math.ldexp(1.0, k)), 0, ONE).astype(np.int64)


def pass_ref(P, f, d, moves, w):
    """One pass with weight w over the valid faces f: every P' from P."""
    S = np.zeros_like(P)
    for j in range(3):
        np.add.at(S, f[:, j], P[f[:, (j + 1) % 3]] + P[f[:, (j + 2) % 3]])
    out = P.copy()
    Pf = P[moves].astype(np.float64)
    mean = S[moves].astype(np.float64) / d[moves].astype(np.float64)[:, None]
    diff = mean - Pf
    prod = np.float64(w) * diff
    out[moves] = np.clip(np.rint(Pf + prod).astype(np.int64), 0, ONE)
    return out


def output_ref(P, lo, k):
    lo = np.asarray(lo, dtype=np.float32).astype(np.float64)
    return (lo + np.ldexp(P.astype(np.float64), -k)).astype(np.float32)


def smooth_ref(vertices, faces, lo, k, steps, lam, mu, pin_border=True):
    V = len(np.asarray(vertices).reshape(-1, 3))
    f = valid_faces(faces, V)
    d, _ = adjacency_ref(faces, V)
    moves = ~pinned_ref(faces, V, pin_border)
    P = quantise_ref(vertices, lo, k)
    for _ in range(steps):
        P = pass_ref(P, f, d, moves, lam)
        P = pass_ref(P, f, d, moves, mu)
    return output_ref(P, lo, k)


def normal_sums_ref(vertices, faces, k2):
    v = np.asarray(vertices, dtype=np.float32).reshape(-1, 3).astype(np.float64)
    f = valid_faces(faces, len(v))
    e1, e2 = v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]]
    c = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2], e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], axis=1)
    q = np.rint(np.clip(c * math.ldexp(1.0, k2), -2.0 ** 62, 2.0 ** 62)).astype(np.int64)
    N = np.zeros((len(v), 3), np.int64)
    for j in range(3):
        np.add.at(N, f[:, j], q)
    return N


def normals_ref(vertices, faces, k2):
    N = normal_sums_ref(vertices, faces, k2)
    x = N.astype(np.float64)
    L = np.sqrt((x[:, 0] * x[:, 0] + x[:, 1] * x[:, 1]) + x[:, 2] * x[:, 2])
    zero = (N == 0).all(axis=1)
    out = np.zeros((len(N), 3), np.float32)
    out[~zero] = (x[~zero] / L[~zero, None]).astype(np.float32)
    return out


def box_of(vertices):
    """(lo, k, k2) as Mesh.smooth works them out: E = the largest extent of the float32 bounding box (0 counts as 1), e = ceil(log2(E)),
    lo_a = (min_a + max_a) / 2 - 2^e in Python floats (the library rounds it to float32), k = 29 - e, k2 = 44 - 2 e."""
    v = np.asarray(vertices, dtype=np.float32).reshape(-1, 3)
    mn, mx = [float(x) for x in v.min(axis=0)], [float(x) for x in v.max(axis=0)]
    E = max(mx[a] - mn[a] for a in range(3))
    e = math.ceil(math.log2(E)) if E > 0 else 0
    assert 2.0 ** (e - 1) < (E if E > 0 else 1.0) <= 2.0 ** e
    return [(mn[a] + mx[a]) / 2 - 2.0 ** e for a in range(3)], 29 - e, 44 - 2 * e


def volume(vertices, faces):
    v = np.asarray(vertices, dtype=np.float64)
    f = valid_faces(faces, len(v))
    return float(np.einsum("ij,ij->i", v[f[:, 0]], np.cross(v[f[:, 1]], v[f[:, 2]])).sum() / 6.0)


# ---------------------------------------------------------------------------------------------------------------- hand cases
# name -> dict(v, f, lo, k, steps, lam, mu, pin, out and what else the case pins): small enough to follow with a pencil.  Unless said, the box
# starts at the origin and k = 4: P = 16 v, so coordinates that are multiples of 1/16 sit on the lattice and `out` is P' / 16.
def _case(v, f, out, steps=1, lam=0.5, mu=0.0, pin=True, lo=(0.0, 0.0, 0.0), k=4, **more):
    return dict(v=np.asarray(v, np.float32).reshape(-1, 3), f=np.asarray(f, np.int32).reshape(-1, 3), lo=lo, k=k, steps=steps, lam=lam, mu=mu,
                pin=pin, out=np.asarray(out, np.float32).reshape(-1, 3), **more)


TRI = [[0, 0, 0], [4, 0, 0], [0, 4, 0]]
# a closed tetrahedron, faces counter-clockwise seen from outside: every vertex has the other three twice, d = 6, h = 0
TET_V = [[1, 1, 1], [5, 1, 1], [1, 5, 1], [1, 1, 5]]
TET_F = [[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]]
# an open fan of four faces around vertex 0, its rim 1..5 not closed: 0 is on the border too (the edges 0-1 and 0-5 are used once)
FAN_V = [[2, 2, 0], [4, 2, 0], [4, 4, 0], [2, 4, 0], [0, 4, 0], [0, 2, 0]]
FAN_F = [[0, 1, 2], [0, 2, 3], [0, 3, 4], [0, 4, 5]]
# a closed fan -- a square pyramid without its base: the apex 0 is interior (d = 8, h = 0), the rim 1..4 is the border
PYR_V = [[2, 2, 4], [0, 0, 0], [4, 0, 0], [4, 4, 0], [0, 4, 0]]
PYR_F = [[0, 1, 2], [0, 2, 3], [0, 3, 4], [0, 4, 1]]

HAND = {
    # with pin_border every vertex of a lone triangle is on the border: nothing moves (the round trip is exact: the corners sit on the lattice)
    "one triangle pinned": _case(TRI, [[0, 1, 2]], TRI, pinned=[1, 1, 1]),
    # without it each corner goes half the way to the mean of the other two: (0,0,0) -> (1,1,0), (4,0,0) -> (2,1,0), (0,4,0) -> (1,2,0)
    "one triangle free": _case(TRI, [[0, 1, 2]], [[1, 1, 0], [2, 1, 0], [1, 2, 0]], pin=False, pinned=[0, 0, 0]),
    # P = 16 v; the mean of the other three, e.g. for vertex 0: (112/3, 112/3, 112/3); P' = rint(16 + 0.5 (37.33 - 16)) = rint(26.67) = 27
    # for vertex 1, x: the others' mean is 16, P' = rint(80 - 32) = 48; y and z: mean (16 + 80 + 16) / 3 = 37.33 -> 27
    "a closed tetrahedron": _case(TET_V, TET_F, np.array([[27, 27, 27], [48, 27, 27], [27, 48, 27], [27, 27, 48]]) / 16.0, pinned=[0, 0, 0, 0]),
    # one step = lambda then mu: from the P' above, vertex 0 with mu = -0.5: mean of the others (34, 34, 34), 27 - 0.5 * 7 = 23.5 -> 24 (ties to
    # even); vertex 1, x: mean 27, 48 + 0.5 * 21 = 58.5 -> 58 (to even); y: mean (27 + 48 + 27) / 3 = 34 -> 23.5 -> 24
    "a closed tetrahedron, a full step": _case(TET_V, TET_F, np.array([[24, 24, 24], [58, 24, 24], [24, 58, 24], [24, 24, 58]]) / 16.0, mu=-0.5),
    "an open fan": _case(FAN_V, FAN_F, FAN_V, pinned=[1, 1, 1, 1, 1, 1]),
    # free, the hub: entries 1, 2, 2, 3, 3, 4, 4, 5 -> S = 16 (4+4+4+2+2+0+0+0, 2+4+4+4+4+4+4+2) = 16 (16, 28), mean (32, 56), P = (32, 32):
    # P' = (32, 44) -> (2, 2.75); vertex 1 has the entries 2 and 0: mean (48, 48), P = (64, 32) -> (56, 40) -> (3.5, 2.5)
    "an open fan, free": _case(FAN_V, FAN_F, [[2, 2.75, 0], [3.5, 2.5, 0], [3.25, 3.25, 0], [2, 3.5, 0], [0.75, 3.25, 0], [0.5, 2.5, 0]], pin=False),
    # the apex moves half the way to the rim's mean (2, 2, 0): (2, 2, 4) -> (2, 2, 2); the rim is pinned
    "a closed fan": _case(PYR_V, PYR_F, [[2, 2, 2]] + PYR_V[1:], pinned=[0, 1, 1, 1, 1]),
    # two closed fans meeting in their apex 0: its link is two cycles, h = 0 + 0: it moves to the mean of both rims, (2, 2, 4) -> (2, 2, 4):
    # the second pyramid is the first mirrored in z = 4, so the mean of the eight rim vertices is the apex itself
    "two fans meeting in one vertex": _case(
        PYR_V + [[0, 0, 8], [4, 0, 8], [4, 4, 8], [0, 4, 8]], PYR_F + [[0, 6, 5], [0, 7, 6], [0, 8, 7], [0, 5, 8]],
        PYR_V + [[0, 0, 8], [4, 0, 8], [4, 4, 8], [0, 4, 8]], pinned=[0] + [1] * 8),
    # the second pyramid lower and given once more: its entries count twice -- apex: 8 entries of the rim z = 0, 16 of the rim z = 6; mean z = 4:
    # nothing moves in z, and x, y stay by symmetry; so the apex is put off-centre: (1, 2, 4) -> x: 16 + 0.5 (32 - 16) = 24 -> 1.5
    "a duplicate face": _case(
        [[1, 2, 4]] + PYR_V[1:] + [[0, 0, 6], [4, 0, 6], [4, 4, 6], [0, 4, 6]], PYR_F + 2 * [[0, 6, 5], [0, 7, 6], [0, 8, 7], [0, 5, 8]],
        [[1.5, 2, 4]] + PYR_V[1:] + [[0, 0, 6], [4, 0, 6], [4, 4, 6], [0, 4, 6]], degrees=[24, 4, 4, 4, 4, 8, 8, 8, 8]),
    # faces with an id outside [0, 5) count for nothing: the closed fan of above
    "invalid ids": _case(PYR_V, [[0, 1, 5], [-1, 1, 2]] + PYR_F + [[2 ** 31 - 1, 0, 1], [0, -2 ** 31, 2]], [[2, 2, 2]] + PYR_V[1:]),
    # vertex 5 is used by no face: d = 0, it stays (without pin_border too: the tests look)
    "an unreferenced vertex": _case(PYR_V + [[3, 1, 2]], PYR_F, [[2, 2, 2]] + PYR_V[1:] + [[3, 1, 2]], degrees=[8, 4, 4, 4, 4, 0],
                                    pinned=[0, 1, 1, 1, 1, 1]),
    # k = 28, the box [0, 4]^3: the rim vertices lie outside it and are moved onto it by the clamp, in the round trip already: (-1, -1, 0) ->
    # (0, 0, 0), (5, -1, 0) -> (4, 0, 0), ...; the apex then moves half the way to the clamped rim's mean (2, 2, 0)
    "the clamp": _case([[2, 2, 4], [-1, -1, 0], [5, -1, 0], [5, 5, 0], [-1, 5, 0]], PYR_F, [[2, 2, 2], [0, 0, 0], [4, 0, 0], [4, 4, 0], [0, 4, 0]], k=28),
    # steps = 0 at the C level: the round trip -- 0.3 is not on the lattice of k = 4: rint(4.8) = 5 -> 0.3125; 2.7 -> rint(43.2) = 43 -> 2.6875
    "steps = 0": _case([[0.3, 1, 2.7], [4, 0, 0], [0, 4, 0]], [[0, 1, 2]], [[0.3125, 1, 2.6875], [4, 0, 0], [0, 4, 0]], steps=0, pin=False),
    # mu = 0: the second pass of the step changes nothing -- the lambda pass of "a closed tetrahedron"
    "mu = 0": _case(TET_V, TET_F, np.array([[27, 27, 27], [48, 27, 27], [27, 48, 27], [27, 27, 48]]) / 16.0, steps=1, lam=0.5, mu=0.0),
    "no faces": _case([[0.3, 1, 2.7], [4, 0, 0]], np.zeros((0, 3)), [[0.3125, 1, 2.6875], [4, 0, 0]], pin=False, degrees=[0, 0]),
}


def hand(name):
    return HAND[name]


def fan(n):
    """A closed fan of n faces around vertex 0 on a cone: the hub above a rim of n vertices on the unit circle, with a little seeded noise."""
    rng = np.random.default_rng(n)
    t = 2 * np.pi * np.arange(n) / n
    rim = np.stack([np.cos(t), np.sin(t), np.zeros(n)], axis=1) + rng.uniform(-0.01, 0.01, (n, 3))
    v = np.concatenate([[[0.05, -0.03, 0.5]], rim]).astype(np.float32)
    i = np.arange(n)
    f = np.stack([np.zeros(n, np.int64), 1 + i, 1 + (i + 1) % n], axis=1).astype(np.int32)
    return v, f

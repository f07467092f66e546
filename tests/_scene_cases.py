"""Float64 numpy restatement of the scene bounds (the arithmetic of DESIGN 3.6 N8, nothing cleverer) and the seeded inputs of the scene
tests.  tests/golden/make_golden_scene.py stores what the reference's PhototourismDataset.read_meta gives on two synthetic COLMAP models."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g18_scene.npz")
INF_BITS = np.uint64(0x7FF0000000000000)
MODELS = {"a": dict(seed=11, n_images=7, n_points=5000, img_downscale=2), "b": dict(seed=12, n_images=3, n_points=1500, img_downscale=1)}


# ---------------------------------------------------------------- the restatement
def depths(xyz, row):
    """((x r20 + y r21) + z r22) + t2: one numpy call per operation, so nothing is fused."""
    xyz = np.asarray(xyz, dtype=np.float64).reshape(-1, 3)
    a = np.multiply(xyz[:, 0], row[0])
    b = np.multiply(xyz[:, 1], row[1])
    c = np.multiply(xyz[:, 2], row[2])
    return np.add(np.add(np.add(a, b), c), row[3])


def in_front(z):
    """0 < bits <= +inf's: positive values, denormals and +inf included; +-0, negatives and NaN are not."""
    b = np.ascontiguousarray(z, dtype=np.float64).view(np.uint64)
    return (b > np.uint64(0)) & (b <= INF_BITS)


def percentile(s, q):
    """np.percentile(s, q) of an ascending float64 array, linear method, written out."""
    n = len(s)
    v = np.float64(q) / np.float64(100) * np.float64(n - 1)
    lo = int(np.floor(v))
    g = v - np.floor(v)
    a, b = np.float64(s[lo]), np.float64(s[min(lo + 1, n - 1)])
    with np.errstate(invalid="ignore", over="ignore"):
        d = b - a
        return a + d * g if g < 0.5 else b - d * (np.float64(1) - g)


def bounds(xyz, rows, q=(0.1, 99.9)):
    """(nears, fars, counts) of every row of rows [N, 4]; NaN and 0 where nothing is in front."""
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, 4)
    nears, fars = np.full(len(rows), np.nan), np.full(len(rows), np.nan)
    counts = np.zeros(len(rows), dtype=np.int32)
    for i, row in enumerate(rows):
        with np.errstate(invalid="ignore", over="ignore"):
            z = depths(xyz, row)
        s = np.sort(z[in_front(z)])
        counts[i] = len(s)
        if len(s):
            nears[i], fars[i] = percentile(s, q[0]), percentile(s, q[1])
    return nears, fars, counts


def same_bits(a, b):
    """Equality of float64 arrays bit for bit, any NaN equal to any NaN."""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint64), b[~nb].view(np.uint64)))


# ---------------------------------------------------------------- seeded inputs
def rotation(q):
    """Rotation matrix of a quaternion (w, x, y, z), normalised first."""
    w, x, y, z = np.asarray(q, dtype=np.float64) / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def generic(seed, n_points, n_images):
    """A blob of points around the origin seen by cameras on a shell around it, some inside the blob: points behind every camera."""
    rng = np.random.default_rng(seed)
    xyz = rng.normal(0.0, 4.0, (n_points, 3))
    rows = np.empty((n_images, 4))
    for i in range(n_images):
        R = rotation(rng.normal(size=4))
        centre = rng.normal(size=3)
        centre *= rng.uniform(0.0, 12.0) / np.linalg.norm(centre)
        rows[i, :3] = R[2]
        rows[i, 3] = -(R[2] @ centre)
    return xyz, rows


AXIS = np.array([0.0, 0.0, 1.0, 0.0])        # row 2 of the identity pose: the depth IS the z coordinate, exactly


def along_z(zs, seed=0):
    """Points whose z coordinates are zs, in a seeded order, with x and y that the AXIS row multiplies by 0."""
    rng = np.random.default_rng(seed)
    zs = np.asarray(zs, dtype=np.float64)
    xyz = np.column_stack([rng.integers(-9, 10, len(zs)).astype(np.float64), rng.integers(-9, 10, len(zs)).astype(np.float64), zs])
    return xyz[rng.permutation(len(zs))]


def shifted(t2s):
    rows = np.tile(AXIS, (len(t2s), 1))
    rows[:, 3] = t2s
    return rows


def edge_cases():
    """name -> (xyz [P, 3], rows [N, 4], q).  Every case is small; the names say what it is there for."""
    rng = np.random.default_rng(5)
    c = {}
    # 10 points at z = -9.5 ... -0.5: t2 = 0, 1, 2 puts 0, 1, 2 of them in front; 20 puts all
    c["count_0_1_2"] = (along_z(np.arange(10) - 9.5), shifted([0.0, 1.0, 2.0, 20.0, -3.0]), (0.1, 99.9))
    for n in (1001, 2001):                       # (n - 1) q / 100 is 1 and 2 (up to its rounding) at q = 0.1
        c["n_%d" % n] = (along_z(np.concatenate([rng.uniform(0.5, 90.0, n), -rng.uniform(0.5, 9.0, 37)]), n), shifted([0.0]), (0.1, 99.9))
    c["q_0_100"] = (generic(21, 777, 3) + ((0.0, 100.0),))
    c["q_equal"] = (generic(22, 300, 2) + ((50.0, 50.0),))
    c["ties"] = (along_z(np.full(1500, 3.25)), shifted([0.0, 1.0, -3.0, -3.25]), (0.1, 99.9))
    # two depths, n = 2000: ranks 1|2 (near) and 1997|1998 (far) straddle the step in one image each
    c["two_depths"] = (along_z(np.concatenate([np.full(2, 1.5), np.full(1998, 7.0)])), shifted([0.0, 0.25]), (0.1, 99.9))
    c["two_depths_far"] = (along_z(np.concatenate([np.full(1998, 1.5), np.full(2, 7.0)])), shifted([0.0, 0.25]), (0.1, 99.9))
    c["one_exponent"] = (along_z(rng.uniform(1.0, 2.0, 3000)), shifted([0.0]), (0.1, 99.9))
    c["one_exponent_low_bits"] = (along_z(1.0 + np.arange(3000) * 2.0 ** -52), shifted([0.0]), (0.1, 99.9))
    # depth exactly +0.0: (1 * 0.5 + 1 * 0.5) + (-2) * 0.5 + 0; exactly -0.0: every product and t2 are -0.0.  Both are excluded.
    zero = np.array([[1.0, 1.0, -2.0], [3.0, -1.0, -2.0], [0.0, 0.0, 0.0], [1.0, 1.0, 1.0], [2.0, 2.0, 2.0], [-1.0, -1.0, -1.0]])
    c["zero_depths"] = (zero, np.array([[0.5, 0.5, 0.5, 0.0], [-0.5, -0.5, -0.5, -0.0], [0.0, 0.0, 0.0, 0.0], [0.0, 0.0, 0.0, -0.0]]), (0.1, 99.9))
    xyz, rows = generic(23, 1200, 4)
    c["nan_free"] = (xyz.copy(), rows, (0.1, 99.9))
    xyz = np.concatenate([xyz[:700], [[np.nan, 1.0, 2.0], [0.5, np.nan, np.nan]], xyz[700:]])
    c["nan_points"] = (xyz, rows, (0.1, 99.9))
    wide = np.concatenate([[5e-324, 1e-320, 2.2250738585072014e-308, 1e300], 10.0 ** rng.uniform(-310, 300, 900), -(10.0 ** rng.uniform(-310, 300, 50))])
    c["denormal_to_1e300"] = (along_z(wide), shifted([0.0]), (0.1, 99.9))
    c["denormal_to_1e300_ends"] = (along_z(wide), shifted([0.0]), (0.0, 100.0))
    c["infinite_depth"] = (along_z([1.0, 2.0, np.inf, np.inf, -np.inf, 3.0]), shifted([0.0]), (0.0, 100.0))
    return c


def hand_case():
    """Identity rotation, integer coordinates: z = 1 ... 5 in front, two behind.  q = (25, 75): v = 1 and 3, so 2 and 4; q = (12.5, 87.5):
    v = 0.5 and 3.5, g = 0.5, so 2 - 0.5 and 5 - 0.5."""
    xyz = np.array([[4.0, -2.0, 3.0], [0.0, 7.0, 1.0], [1.0, 1.0, -1.0], [-3.0, 0.0, 5.0], [2.0, 2.0, 2.0], [9.0, 9.0, -2.0], [0.0, 0.0, 4.0]])
    return xyz, AXIS[None].copy(), {(25.0, 75.0): (2.0, 4.0), (12.5, 87.5): (1.5, 4.5)}, 5


# ---------------------------------------------------------------- the synthetic COLMAP models of the golden file
def colmap_model(seed, n_images, n_points, **_):
    """What make_golden_scene.py writes into cameras.bin / images.bin / points3D.bin: ids (camera id = image id), unit quaternions,
    translations, PINHOLE parameters and points.  The cameras look at a blob, some from inside it: points behind them."""
    rng = np.random.default_rng(seed)
    ids = np.sort(rng.choice(np.arange(1, 60), n_images, replace=False)).astype(np.int64)
    xyz = rng.normal(0.0, 3.0, (n_points, 3)) * np.array([1.0, 0.6, 1.0])
    qvecs, tvecs = np.empty((n_images, 4)), np.empty((n_images, 3))
    for i in range(n_images):
        q = rng.normal(size=4)
        q /= np.linalg.norm(q)
        R = rotation(q)
        centre = -R[2] * rng.uniform(1.0, 30.0) + rng.normal(0.0, 1.0, 3)        # behind the blob along the view axis, or inside it
        qvecs[i], tvecs[i] = q, -R @ centre
    wh = rng.integers(300, 1100, (n_images, 2))
    params = np.column_stack([rng.uniform(400, 1500, n_images), rng.uniform(400, 1500, n_images), wh[:, 0] / 2.0, wh[:, 1] / 2.0])
    return dict(ids=ids, qvecs=qvecs, tvecs=tvecs, params=params, xyz=xyz)


def load_golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def depth_error_bound(xyz, row):
    """Per point, the most two evaluations of the 4-term sum x r20 + y r21 + z r22 + t2 can differ by, whatever their order and fusing:
    8 * 2^-53 * (|x r20| + |y r21| + |z r22| + |t2|)."""
    return 8 * 2.0 ** -53 * (np.abs(xyz[:, 0] * row[0]) + np.abs(xyz[:, 1] * row[1]) + np.abs(xyz[:, 2] * row[2]) + abs(row[3]))

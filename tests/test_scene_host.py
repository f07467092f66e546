"""CPU-only: the host half of crnerf_amd.datasets.scene against what the reference's read_meta recorded on two synthetic COLMAP models
(tests/golden/g18_scene.npz), the numpy restatement of the scene bounds (tests/_scene_cases.py) against np.percentile and against the
reference's own depth expression, and the argument checks of the device entry point."""
import numpy as np
import pytest
import torch

import _scene_cases as S
from crnerf_amd import ops
from crnerf_amd.datasets import scene


@pytest.fixture(scope="module")
def models():
    g = S.load_golden()
    out = {}
    for key, spec in S.MODELS.items():
        m = {k[len(key) + 1:]: v for k, v in g.items() if k.startswith(key + "_")}
        m["img_downscale"] = spec["img_downscale"]
        m["w2c"] = scene.world_to_camera(m["qvecs"], m["tvecs"])
        m["bounds"] = S.bounds(m["xyz"], m["w2c"][:, 2, :])                # unscaled (nears, fars, counts) of the restatement, computed once
        out[key] = m
    return out


def restated_scale(m):
    """float32(max far) / 5 in float32, from the restatement's fars."""
    return np.float32(m["bounds"][1].astype(np.float32).max() / np.float32(5))


def test_golden_is_what_the_seeds_give(models):
    """The stored raw arrays are the seeded models in the .tsv's order, and the sizes are the ones asked for."""
    for key, spec in S.MODELS.items():
        m, raw = models[key], S.colmap_model(**spec)
        assert m["img_ids"].shape == (spec["n_images"],) and m["xyz"].shape == (spec["n_points"], 3)
        order = [int(np.flatnonzero(raw["ids"] == i)[0]) for i in m["img_ids"]]
        assert sorted(order) == list(range(spec["n_images"])) and order != sorted(order)
        for name in ("qvecs", "tvecs", "params"):
            assert np.array_equal(raw[name][order], m[name])
        assert np.array_equal(raw["xyz"], m["xyz"])


@pytest.mark.parametrize("key", sorted(S.MODELS))
def test_scaled_intrinsics_bit_for_bit(models, key):
    m = models[key]
    K = scene.scaled_intrinsics(m["params"], m["img_downscale"])
    assert K.dtype == np.float32 and K.shape == m["Ks"].shape
    assert np.array_equal(K.view(np.uint32), m["Ks"].view(np.uint32))
    assert np.array_equal(scene.scaled_intrinsics(torch.from_numpy(m["params"]), m["img_downscale"]), K)


def test_scaled_intrinsics_rejects_what_is_not_pinhole():
    for bad in (np.zeros((3, 3)), np.zeros((3, 5)), np.zeros(4), np.zeros((2, 4, 1))):
        with pytest.raises(ValueError, match="PINHOLE"):
            scene.scaled_intrinsics(bad, 2)
    with pytest.raises(ValueError, match="image 1"):
        scene.scaled_intrinsics(np.array([[500.0, 500.0, 320.0, 240.0], [500.0, 500.0, 0.25, 240.0]]), 2)
    with pytest.raises(ValueError, match="image 0"):
        scene.scaled_intrinsics(np.array([[np.nan, 500.0, 320.0, 240.0]]), 1)
    with pytest.raises(ValueError, match="img_downscale"):
        scene.scaled_intrinsics(np.array([[500.0, 500.0, 320.0, 240.0]]), 0)


def test_rotation_and_world_to_camera():
    rng = np.random.default_rng(3)
    q = rng.normal(size=(9, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    t = rng.normal(size=(9, 3))
    R = scene.qvec2rotmat(q)
    assert R.shape == (9, 3, 3) and R.dtype == np.float64
    for i in range(9):
        assert np.array_equal(scene.qvec2rotmat(q[i]), R[i])
        assert np.abs(R[i] - S.rotation(q[i])).max() < 1e-15
        assert np.abs(R[i] @ R[i].T - np.eye(3)).max() < 1e-15 and abs(np.linalg.det(R[i]) - 1) < 1e-15
    assert np.array_equal(scene.qvec2rotmat([1.0, 0.0, 0.0, 0.0]), np.eye(3))
    w2c = scene.world_to_camera(q, t)
    assert w2c.shape == (9, 4, 4) and np.array_equal(w2c[:, :3, :3], R) and np.array_equal(w2c[:, :3, 3], t)
    assert np.array_equal(w2c[:, 3], np.tile([0.0, 0.0, 0.0, 1.0], (9, 1)))
    with pytest.raises(ValueError):
        scene.world_to_camera(q, t[:5])
    with pytest.raises(ValueError):
        scene.qvec2rotmat(np.zeros(3))


@pytest.mark.parametrize("key", sorted(S.MODELS))
def test_poses_and_scale(models, key):
    """camera_poses and the scaled poses to 1e-12 of the largest element (np.linalg.inv is LAPACK's: the last bits may differ between
    builds; the measured difference is printed, 0 where this was written); the scale bit for bit -- the stored xyz_world is the raw
    points divided by it in float64, which no other float32 reproduces."""
    m = models[key]
    s = restated_scale(m)
    assert s.dtype == np.float32
    assert np.array_equal((m["xyz"] / np.float64(s)).view(np.uint64), m["xyz_world"].view(np.uint64))
    poses = scene.camera_poses(m["w2c"])
    assert poses.shape == m["poses"].shape and poses.dtype == np.float64
    big = np.abs(m["poses"][..., :3]).max()
    d_rot = np.abs(poses[..., :3] - m["poses"][..., :3]).max()
    scaled = poses.copy()
    scaled[..., 3] /= np.float64(s)
    d_all = np.abs(scaled - m["poses"]).max()
    print("model %s: max |d rotation| %.3g, max |d scaled pose| %.3g, largest element %.3g" % (key, d_rot, d_all, np.abs(m["poses"]).max()))
    assert d_rot <= 1e-12 * big and d_all <= 1e-12 * np.abs(m["poses"]).max()
    # what the inverse has to be: R^T and the camera centre, columns 1 and 2 negated
    for i in range(len(poses)):
        R, t = m["w2c"][i, :3, :3], m["w2c"][i, :3, 3]
        want = np.concatenate([R.T, (-R.T @ t)[:, None]], 1)
        want[:, 1:3] *= -1
        assert np.abs(poses[i] - want).max() <= 1e-12 * max(1.0, np.abs(want).max())


def percentile_cases():
    cases = [(name,) + c for name, c in S.edge_cases().items()]
    cases += [("generic_%d_%d" % (p, n), *S.generic(100 + p + n, p, n), (0.1, 99.9)) for p, n in ((1, 3), (2, 3), (257, 3), (5000, 7))]
    return cases


@pytest.mark.parametrize("case", percentile_cases(), ids=lambda c: c[0])
def test_restated_percentile_is_numpys(case):
    name, xyz, rows, q = case
    nears, fars, counts = S.bounds(xyz, rows, q)
    for i, row in enumerate(rows):
        with np.errstate(invalid="ignore", over="ignore"):
            z = S.depths(xyz, row)
            z = z[z > 0]                                    # numpy's own filter, as the reference writes it
            assert len(z) == counts[i]
            if len(z) == 0:
                assert np.isnan(nears[i]) and np.isnan(fars[i])
                continue
            assert S.same_bits(nears[i], np.percentile(z, q[0])) and S.same_bits(fars[i], np.percentile(z, q[1])), (name, i)


def test_restated_percentile_on_random_lengths():
    rng = np.random.default_rng(8)
    for _ in range(300):
        n = int(rng.integers(1, 3000))
        s = np.sort(rng.uniform(0.0, 10.0 ** rng.uniform(-3, 3), n))
        q = float(rng.choice([0.0, 0.1, 25.0, 50.0, 99.9, 100.0, rng.uniform(0, 100)]))
        assert S.same_bits(S.percentile(s, q), np.percentile(s, q)), (n, q)


def test_in_front_is_decided_on_the_bits():
    z = np.array([0.0, -0.0, 5e-324, -5e-324, 1.0, -1.0, np.inf, -np.inf, np.nan, -np.nan, 2.2250738585072014e-308])
    assert S.in_front(z).tolist() == [False, False, True, False, True, False, True, False, False, False, True]
    with np.errstate(invalid="ignore"):
        assert np.array_equal(S.in_front(z), z > 0)


def test_hand_case_of_the_restatement():
    xyz, rows, want, n = S.hand_case()
    for q, (near, far) in want.items():
        nears, fars, counts = S.bounds(xyz, rows, q)
        assert nears[0] == near and fars[0] == far and counts[0] == n


@pytest.mark.parametrize("key", sorted(S.MODELS))
def test_stored_bounds_within_the_depth_error_bound(models, key):
    """Our depth ((x r20 + y r21) + z r22) + t2 and the reference's (xyz_h @ w2c.T)[:, 2] are two evaluations of one 4-term sum: they differ
    by at most 8 * 2^-53 * (|x r20| + |y r21| + |z r22| + |t2|) per point (measured, in those units, below).  No depth of a golden model
    lies within that of 0, so both sides count the same points, order statistics move by no more than their inputs, and the stored nears
    and fars are held to the image's largest bound, divided by the scale."""
    m = models[key]
    xyz, w2c = m["xyz"], m["w2c"]
    nears, fars, counts = m["bounds"]
    s = np.float64(restated_scale(m))
    xyz_h = np.concatenate([xyz, np.ones((len(xyz), 1))], -1)
    for i in range(len(w2c)):
        ours = S.depths(xyz, w2c[i, 2])
        theirs = (xyz_h @ w2c[i].T)[:, 2]
        bound = S.depth_error_bound(xyz, w2c[i, 2])
        assert np.abs(ours).min() > bound.max(), "a depth within the bound of 0: the two sides may count different points"
        assert counts[i] == int((theirs > 0).sum())
        units = (np.abs(ours - theirs) / (bound / 8)).max()
        d_near, d_far = abs(nears[i] / s - m["nears"][i]), abs(fars[i] / s - m["fars"][i])
        print("model %s image %d: n %d, depths differ by <= %.2f of 2^-53 * sum|terms|, |d near| %.3g, |d far| %.3g, bound %.3g"
              % (key, i, counts[i], units, d_near, d_far, bound.max() / s))
        assert np.all(np.abs(ours - theirs) <= bound)
        assert d_near <= bound.max() / s and d_far <= bound.max() / s
    assert abs(m["fars"].max() - 5.0) < 5 * 2.0 ** -23          # the largest far is 5 up to the float32 rounding of the scale


def test_device_entry_points_refuse_host_tensors_and_float32():
    xyz, rows = torch.zeros(4, 3, dtype=torch.float64), torch.zeros(2, 4, dtype=torch.float64)
    with pytest.raises(ValueError, match="GPU"):
        ops.scene_bounds(xyz, rows)
    with pytest.raises(TypeError, match="float64"):
        scene.depth_bounds(np.zeros((4, 3), dtype=np.float32), np.zeros((2, 4, 4)))
    with pytest.raises(TypeError, match="float64"):
        scene.depth_bounds(np.zeros((4, 3)), torch.zeros(2, 4, 4, dtype=torch.float32))


def test_abi_rejects_wrong_arguments_before_any_device_work():
    """crnerf_scene_bounds_f64 returns the library's error codes for null pointers, n_images < 1, n_points < 0, a percentile outside
    [0, 100] (NaN included) and q_lo > q_hi; crnerf_scene_bounds_workspace_bytes is 0 -- the histograms are on chip, no depth is stored --
    which is why ops.scene_bounds passes no workspace (tests/test_gpu_scene.py runs it that way)."""
    from crnerf_amd import _lib
    lib = _lib.load()
    for n, p in ((1, 0), (1, 1), (7, 5000), (1024, 200000), (300, 2 ** 31 - 1)):
        assert lib.crnerf_scene_bounds_workspace_bytes(n, p) == 0
    assert lib.crnerf_scene_bounds_workspace_bytes(0, 10) == 0 and lib.crnerf_scene_bounds_workspace_bytes(3, -1) == 0
    p = 4096                                             # a non-null value: never dereferenced on these paths
    call = lambda *a: lib.crnerf_scene_bounds_f64(*a, None, None)  # noqa: E731  (no workspace, the null stream)
    assert call(None, 10, p, 3, 0.1, 99.9, p, p, p) == -1
    assert b"NULL" in lib.crnerf_last_error()
    assert call(p, 10, None, 3, 0.1, 99.9, p, p, p) == -1
    assert call(p, 10, p, 3, 0.1, 99.9, None, p, p) == -1
    assert call(p, 10, p, 3, 0.1, 99.9, p, None, p) == -1
    assert call(p, 10, p, 3, 0.1, 99.9, p, p, None) == -1
    assert call(p, 10, p, 0, 0.1, 99.9, p, p, p) == -2
    assert call(p, 10, p, -4, 0.1, 99.9, p, p, p) == -2
    assert call(p, -1, p, 3, 0.1, 99.9, p, p, p) == -2
    assert call(p, 10, p, 3, -1.0, 99.9, p, p, p) == -3
    assert b"percentile" in lib.crnerf_last_error()
    assert call(p, 10, p, 3, 0.1, 101.0, p, p, p) == -3
    assert call(p, 10, p, 3, 101.0, 101.0, p, p, p) == -3
    assert call(p, 10, p, 3, float("nan"), 99.9, p, p, p) == -3
    assert call(p, 10, p, 3, 0.1, float("inf"), p, p, p) == -3
    assert call(p, 10, p, 3, 60.0, 40.0, p, p, p) == -3
    assert b"q_lo" in lib.crnerf_last_error()

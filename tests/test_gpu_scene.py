"""crnerf_scene_bounds_f64 (csrc/scenebounds.hip) and crnerf_amd.datasets.scene on the GPU.  Every comparison with the numpy restatement
(tests/_scene_cases.py, pinned to np.percentile and to the reference's recorded results by tests/test_scene_host.py) is equality of the
float64 bits, NaN equal to NaN, and equality of the counts.  There is no tolerance on the kernel in this file.

Sizes: P = 1, 2, one below / at / one above the workgroup's 256 threads, 1000, 5000; N = 1, 7, 300 workgroups; one 200,000-point model.
Cases: the table of _scene_cases.edge_cases (0, 1 and 2 points in front, integer virtual indices, q = (0, 100), ties, two depths with the
rank boundary between them, one exponent, +0.0 and -0.0 depths, NaN coordinates, denormals to 1e300, +inf) and one written out by hand."""
import numpy as np
import pytest
import torch

import _scene_cases as S
from crnerf_amd import ops
from crnerf_amd.datasets import images, scene

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T = torch.from_numpy

SIZES = [(1, 3), (2, 3), (255, 3), (256, 3), (257, 3), (1000, 3), (5000, 1), (5000, 7), (5000, 300), (200000, 16)]
EDGE = S.edge_cases()
_cache = {}


def device_bounds(xyz, rows, q):
    n, f, c = ops.scene_bounds(T(np.ascontiguousarray(xyz)).to(DEV), T(np.ascontiguousarray(rows)).to(DEV), q[0], q[1])
    assert n.dtype == torch.float64 and f.dtype == torch.float64 and c.dtype == torch.int32
    assert n.shape == f.shape == c.shape == (len(rows),) and n.is_cuda and f.is_cuda and c.is_cuda
    return n.cpu().numpy(), f.cpu().numpy(), c.cpu().numpy()


def check(xyz, rows, q, want=None):
    want = S.bounds(xyz, rows, q) if want is None else want
    got = device_bounds(xyz, rows, q)
    assert np.array_equal(got[2], want[2]), (got[2], want[2])
    bad = [i for i in range(len(rows)) if not (S.same_bits(got[0][i], want[0][i]) and S.same_bits(got[1][i], want[1][i]))]
    assert not bad, "images %s: got %s / %s, want %s / %s" % (bad[:5], got[0][bad[:5]], got[1][bad[:5]], want[0][bad[:5]], want[1][bad[:5]])
    return got


def golden_models():
    if "golden" not in _cache:
        g = S.load_golden()
        _cache["golden"] = {key: dict({k[len(key) + 1:]: v for k, v in g.items() if k.startswith(key + "_")}, img_downscale=spec["img_downscale"])
                            for key, spec in S.MODELS.items()}
    return _cache["golden"]


def prepared(key):
    if ("scene", key) not in _cache:
        m = golden_models()[key]
        _cache[("scene", key)] = scene.prepare_scene(m["qvecs"], m["tvecs"], m["params"], m["xyz"], m["img_downscale"], img_ids=m["img_ids"])
    return _cache[("scene", key)]


@pytest.mark.parametrize("n_points,n_images", SIZES, ids=lambda v: str(v))
def test_sizes(n_points, n_images):
    xyz, rows = S.generic(1000 + n_points + n_images, n_points, n_images)
    got = check(xyz, rows, (0.1, 99.9))
    if n_points >= 1000:
        assert got[2].min() > 0 and (got[2] < n_points).any()         # points in front of every camera, points behind some


@pytest.mark.parametrize("name", sorted(EDGE))
def test_edge_cases(name):
    xyz, rows, q = EDGE[name]
    check(xyz, rows, q)


def test_counts_zero_one_two():
    xyz, rows, q = EDGE["count_0_1_2"]
    nears, fars, counts = device_bounds(xyz, rows, q)
    assert counts.tolist() == [0, 1, 2, 10, 0]
    assert np.isnan(nears[[0, 4]]).all() and np.isnan(fars[[0, 4]]).all()
    assert nears[1] == 0.5 and fars[1] == 0.5                          # one point: both percentiles are its depth
    assert 0.5 <= nears[2] < fars[2] <= 1.5


def test_zero_depths_are_excluded():
    xyz, rows, q = EDGE["zero_depths"]
    with np.errstate(invalid="ignore"):
        z = np.stack([S.depths(xyz, r) for r in rows])
    assert (z[0, :2] == 0).all() and not np.signbit(z[0, :2]).any()    # exactly +0.0
    assert (z[1, 2] == 0) and np.signbit(z[1, 2]) and np.signbit(z[3]).any() and (z[2:] == 0).all()      # exactly -0.0
    assert device_bounds(xyz, rows, q)[2].tolist() == [2, 1, 0, 0]


def test_nan_points_change_nothing():
    (xa, rows, q), (xb, _, _) = EDGE["nan_free"], EDGE["nan_points"]
    a, b = device_bounds(xa, rows, q), device_bounds(xb, rows, q)
    assert np.array_equal(a[2], b[2]) and S.same_bits(a[0], b[0]) and S.same_bits(a[1], b[1]) and not np.isnan(a[0]).any()
    # a NaN in one image's pose leaves the other images alone
    bad = rows.copy()
    bad[1, 3] = np.nan
    c = device_bounds(xa, bad, q)
    assert c[2][1] == 0 and np.isnan(c[0][1]) and np.isnan(c[1][1])
    keep = [0, 2, 3]
    assert np.array_equal(c[2][keep], a[2][keep]) and S.same_bits(c[0][keep], a[0][keep]) and S.same_bits(c[1][keep], a[1][keep])


def test_by_hand():
    xyz, rows, want, n = S.hand_case()
    for q, (near, far) in want.items():
        nears, fars, counts = device_bounds(xyz, rows, q)
        assert (nears[0], fars[0], counts[0]) == (near, far, n)


def test_repeated_calls_agree():
    xyz, rows = S.generic(77, 5000, 7)
    x, r = T(xyz).to(DEV), T(rows).to(DEV)
    a = [t.clone() for t in ops.scene_bounds(x, r)]
    b = ops.scene_bounds(x, r)
    for u, v in zip(a, b):
        assert torch.equal(u.view(torch.int64) if u.dtype == torch.float64 else u, v.view(torch.int64) if v.dtype == torch.float64 else v)


def test_depth_bounds_host_and_device_inputs_agree():
    m = golden_models()["a"]
    w2c = scene.world_to_camera(m["qvecs"], m["tvecs"])
    host = scene.depth_bounds(m["xyz"], w2c)
    x, w = T(m["xyz"]).to(DEV), T(w2c).to(DEV)
    dev = scene.depth_bounds(x, w)
    mixed = scene.depth_bounds(T(m["xyz"]), w)                         # a host tensor beside a device tensor
    want = S.bounds(m["xyz"], w2c[:, 2, :])
    for got in (host, dev, mixed):
        assert got[0].is_cuda and got[0].dtype == torch.float64 and got[2].dtype == torch.int32
        assert S.same_bits(got[0].cpu().numpy(), want[0]) and S.same_bits(got[1].cpu().numpy(), want[1])
        assert np.array_equal(got[2].cpu().numpy(), want[2])
    with pytest.raises(TypeError, match="float64"):
        scene.depth_bounds(x.float(), w)
    with pytest.raises(ValueError):
        ops.scene_bounds(x, w[:, 2, :].contiguous(), 60.0, 40.0)


@pytest.mark.parametrize("key", sorted(S.MODELS))
def test_prepare_scene_reproduces_read_meta(key):
    """tests/test_scene_host.py's comparisons, end to end through prepare_scene: Ks and the scale bit for bit, poses to 1e-12 of the
    largest element, nears and fars within the image's depth error bound divided by the scale."""
    m, sc = golden_models()[key], prepared(key)
    assert np.array_equal(sc.Ks.view(np.uint32), m["Ks"].view(np.uint32))
    assert sc.scale_factor.dtype == np.float32
    assert np.array_equal(sc.xyz_world.view(np.uint64), m["xyz_world"].view(np.uint64))         # only the reference's float32 scale gives these
    assert np.array_equal((m["xyz"] / np.float64(sc.scale_factor)).view(np.uint64), m["xyz_world"].view(np.uint64))
    d_pose = np.abs(sc.poses - m["poses"]).max()
    print("model %s: max |d pose| %.3g" % (key, d_pose))
    assert d_pose <= 1e-12 * np.abs(m["poses"]).max()
    w2c = scene.world_to_camera(m["qvecs"], m["tvecs"])
    s = np.float64(sc.scale_factor)
    for i in range(len(w2c)):
        bound = S.depth_error_bound(m["xyz"], w2c[i, 2]).max() / s
        d_near, d_far = abs(sc.nears[i] - m["nears"][i]), abs(sc.fars[i] - m["fars"][i])
        print("model %s image %d: |d near| %.3g, |d far| %.3g, bound %.3g" % (key, i, d_near, d_far, bound))
        assert d_near <= bound and d_far <= bound
    assert abs(sc.fars.max() - 5.0) < 5 * 2.0 ** -23
    assert sc.nears.dtype == np.float64 and sc.fars.dtype == np.float64 and np.array_equal(sc.img_ids, m["img_ids"])


def test_prepare_scene_names_the_image_with_nothing_in_front():
    m = golden_models()["b"]
    tvecs = m["tvecs"].copy()
    tvecs[1, 2] = -1e6                                                  # pushes every point behind camera 1
    with pytest.raises(ValueError, match=r"image\(s\) \[1\]"):
        scene.prepare_scene(m["qvecs"], tvecs, m["params"], m["xyz"], 1)


def test_scene_feeds_the_image_builders():
    """train_buffer_args and eval_sample_args are the arguments of images.build_train_buffers and images.make_eval_sample: the near and far
    columns of the rays are the scaled bounds cast to float32, the id column the image ids."""
    sc = prepared("a")
    rng = np.random.default_rng(4)
    photos = [rng.integers(0, 256, (31, 47, 3), dtype=np.uint8) for _ in range(2)]
    idx = [5, 2]
    all_rays, all_rgbs, all_imgs_wh, all_imgs = images.build_train_buffers(photos, *sc.train_buffer_args(idx))
    w, h = 47 // 2, 31 // 2
    assert all_rays.shape == (2 * w * h, 9) and all_rgbs.shape == (2 * w * h, 3) and len(all_imgs) == 2
    assert all_imgs_wh.tolist() == [[w, h], [w, h]]
    for k, i in enumerate(idx):
        rows = all_rays[k * w * h:(k + 1) * w * h].cpu()
        assert (rows[:, 6] == float(np.float32(sc.nears[i]))).all() and (rows[:, 7] == float(np.float32(sc.fars[i]))).all()
        assert (rows[:, 8] == float(sc.img_ids[i])).all()
        assert torch.equal(rows[:, :3], T(sc.poses[i][:, 3].astype(np.float32)).expand(w * h, 3))
    sample = images.make_eval_sample(photos[0], *sc.eval_sample_args(3))
    assert sample["rays"].shape == (w * h, 8) and sample["rgbs"].shape == (w * h, 3) and sample["img_wh"].tolist() == [w, h]
    rays = sample["rays"].cpu()
    assert (rays[:, 6] == float(np.float32(sc.nears[3]))).all() and (rays[:, 7] == float(np.float32(sc.fars[3]))).all()
    assert (sample["ts"] == int(sc.img_ids[3])).all()
    assert sample["c2w"].dtype == torch.float32 and torch.equal(sample["c2w"], T(sc.poses[3].astype(np.float32)))
    everything = sc.train_buffer_args()
    assert len(everything[0]) == len(sc.Ks) and everything[4] == sc.img_ids.tolist() and everything[5] == 2

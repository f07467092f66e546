"""Scene preparation of the reference's datasets: the arithmetic of PhototourismDataset.read_meta
(datasets/phototourism_mask_grid_sample.py:85-147) between the parsed COLMAP arrays and what the renderer and the batcher consume -- the
intrinsics scaled to the training size, the camera-to-world poses in "right up back" orientation, one near and one far bound per image
(the 0.1 and 99.9 percentile of the camera-space depth of every point of the sparse model in front of that camera) and the scene scale
max_far / 5 applied to all of them.  The images x points depth pass and its percentiles run on the device (csrc/scenebounds.hip; the
arithmetic is stated in include/crnerf.h and DESIGN 3.6 N8); everything else is a few float64 numpy lines per image.

Parsing cameras.bin, images.bin, points3D.bin and the .tsv stays with the caller: this module starts from their arrays --
per image the quaternion `qvec` (w, x, y, z) and translation `tvec` of images.bin, the PINHOLE `params` (fx, fy, cx, cy) of the image's
camera in cameras.bin, and the `xyz` of every point of points3D.bin, all float64 as COLMAP stores them.

Host-only at import: the HIP library is loaded by the first depth_bounds / prepare_scene call."""
import dataclasses

import numpy as np
import torch


def _host_f64(a, name, tail):
    a = np.asarray(a.detach().cpu() if torch.is_tensor(a) else a)
    if a.dtype != np.float64:
        a = a.astype(np.float64)
    if a.ndim != len(tail) + 1 or tuple(a.shape[1:]) != tuple(tail):
        raise ValueError("crnerf_amd.datasets.scene: %s must have shape [N, %s], got %s" % (name, ", ".join(str(v) for v in tail), a.shape))
    return a


def qvec2rotmat(qvec):
    """COLMAP's rotation matrix of a quaternion (w, x, y, z), float64 [3, 3] (a [N, 4] array gives [N, 3, 3]); not normalised, as COLMAP's
    own helper: the quaternions of images.bin are unit already."""
    q = np.asarray(qvec, dtype=np.float64)
    if q.shape[-1] != 4:
        raise ValueError("crnerf_amd.datasets.scene: a quaternion has 4 components, got shape %s" % (q.shape,))
    w, x, y, z = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    R = np.empty(q.shape[:-1] + (3, 3), dtype=np.float64)
    R[..., 0, 0] = 1.0 - 2.0 * (y * y) - 2.0 * (z * z)
    R[..., 0, 1] = 2.0 * x * y - 2.0 * w * z
    R[..., 0, 2] = 2.0 * z * x + 2.0 * w * y
    R[..., 1, 0] = 2.0 * x * y + 2.0 * w * z
    R[..., 1, 1] = 1.0 - 2.0 * (x * x) - 2.0 * (z * z)
    R[..., 1, 2] = 2.0 * y * z - 2.0 * w * x
    R[..., 2, 0] = 2.0 * z * x - 2.0 * w * y
    R[..., 2, 1] = 2.0 * y * z + 2.0 * w * x
    R[..., 2, 2] = 1.0 - 2.0 * (x * x) - 2.0 * (y * y)
    return R


def world_to_camera(qvecs, tvecs):
    """[N, 4, 4] float64: [[R, t], [0, 0, 0, 1]] per image, R = qvec2rotmat(qvec) (:108-115)."""
    qvecs, tvecs = _host_f64(qvecs, "qvecs", (4,)), _host_f64(tvecs, "tvecs", (3,))
    if len(qvecs) != len(tvecs):
        raise ValueError("crnerf_amd.datasets.scene: %d quaternions but %d translations" % (len(qvecs), len(tvecs)))
    w2c = np.zeros((len(qvecs), 4, 4), dtype=np.float64)
    w2c[:, :3, :3] = qvec2rotmat(qvecs)
    w2c[:, :3, 3] = tvecs
    w2c[:, 3, 3] = 1.0
    return w2c


def camera_poses(w2c):
    """[N, 3, 4] float64, unscaled: np.linalg.inv(w2c)[:, :3] with columns 1 and 2 negated -- COLMAP's "right down front" camera axes
    turned into the renderer's "right up back" (:116-118)."""
    w2c = _host_f64(w2c, "w2c", (4, 4))
    poses = np.array(np.linalg.inv(w2c)[:, :3])
    poses[..., 1:3] *= -1
    return poses


def scaled_intrinsics(params, img_downscale):
    """[N, 3, 3] float32 K per image from the PINHOLE parameters (fx, fy, cx, cy) of its camera (:93-101): the image is int(2 cx) x int(2 cy),
    the training size that // img_downscale, and every parameter is scaled by its axis' (training size / full size) in float64 before the
    store to float32."""
    p = np.asarray(params.detach().cpu() if torch.is_tensor(params) else params)
    if p.ndim != 2 or p.shape[1] != 4:
        raise ValueError("crnerf_amd.datasets.scene: scaled_intrinsics takes the four PINHOLE parameters (fx, fy, cx, cy) per image, shape [N, 4]; "
                         "got shape %s (SIMPLE_PINHOLE, the RADIAL / OPENCV models and their distortion terms are not handled: undistort "
                         "with COLMAP first, as the reference's dense/ model is)" % (p.shape,))
    p = p.astype(np.float64)
    d = int(img_downscale)
    if d < 1 or d != img_downscale:
        raise ValueError("crnerf_amd.datasets.scene: img_downscale must be an integer >= 1, got %r" % (img_downscale,))
    full = np.trunc(p[:, 2:4] * 2)                    # int(cx * 2), int(cy * 2)
    if not np.all(np.isfinite(p)) or np.any(full < 1):
        bad = int(np.flatnonzero(~np.isfinite(p).all(axis=1) | (full < 1).any(axis=1))[0])
        raise ValueError("crnerf_amd.datasets.scene: image %d has PINHOLE parameters %s: not finite, or a principal point that gives an "
                         "empty image" % (bad, p[bad].tolist()))
    small = np.floor_divide(full, d)
    K = np.zeros((len(p), 3, 3), dtype=np.float32)
    K[:, 0, 0] = p[:, 0] * small[:, 0] / full[:, 0]
    K[:, 1, 1] = p[:, 1] * small[:, 1] / full[:, 1]
    K[:, 0, 2] = p[:, 2] * small[:, 0] / full[:, 0]
    K[:, 1, 2] = p[:, 3] * small[:, 1] / full[:, 1]
    K[:, 2, 2] = 1
    return K


def _require_f64(a, name):
    dtype = a.dtype if torch.is_tensor(a) else np.asarray(a).dtype
    if dtype not in (torch.float64, np.float64):
        raise TypeError("crnerf_amd.datasets.scene: %s must be float64, got %s (the bounds are percentiles of float64 depths; float32 is not "
                        "promoted silently: convert it yourself if that is meant)" % (name, dtype))


def _device_f64(a, device):
    """A float64 array as a contiguous device tensor: a device tensor is used in place, a host array is uploaded once."""
    if torch.is_tensor(a):
        return (a if a.is_cuda else a.to(device)).contiguous()
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def depth_bounds(xyz_world, w2c, q=(0.1, 99.9)):
    """(nears float64 [N], fars float64 [N], counts int32 [N]) on the device: per image np.percentile(depth[depth > 0], q[0]) and (..., q[1])
    of the depth ((x r20 + y r21) + z r22) + t2 of every point (:133-137), and how many points lie in front.  xyz_world: float64 [P, 3];
    w2c: float64 [N, 4, 4] world-to-camera matrices.  Host arrays are uploaded once, device tensors are used in place;
    float32 is refused.  An image with nothing in front of it has count 0 and NaN bounds."""
    from .. import ops
    _require_f64(xyz_world, "xyz_world")
    _require_f64(w2c, "w2c")
    dev = next((t.device for t in (xyz_world, w2c) if torch.is_tensor(t) and t.is_cuda), None)
    if dev is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    xyz = _device_f64(xyz_world, dev)
    w = _device_f64(w2c, dev)
    if xyz.dim() != 2 or xyz.shape[1] != 3:
        raise ValueError("crnerf_amd.datasets.scene: xyz_world must have shape [P, 3], got %s" % (tuple(xyz.shape),))
    if w.dim() != 3 or w.shape[1] != 4 or w.shape[2] != 4:
        raise ValueError("crnerf_amd.datasets.scene: w2c must have shape [N, 4, 4], got %s" % (tuple(w.shape),))
    return ops.scene_bounds(xyz, w[:, 2, :].contiguous(), q[0], q[1])


@dataclasses.dataclass
class Scene:
    """read_meta's attributes for the images given, in the order given, after the scene scale."""
    Ks: np.ndarray             # [N, 3, 3] float32, scaled by img_downscale
    poses: np.ndarray          # [N, 3, 4] float64 camera-to-world, translation divided by scale_factor
    nears: np.ndarray          # [N] float64, divided by scale_factor
    fars: np.ndarray           # [N] float64, divided by scale_factor: the largest is 5 up to float32 rounding
    xyz_world: np.ndarray      # [P, 3] float64, divided by scale_factor
    scale_factor: np.float32   # float32(max far) / 5
    img_ids: np.ndarray        # [N] int64: the ids the rays carry (prepare_scene's img_ids, default 0 .. N-1)
    img_downscale: int

    def train_buffer_args(self, indices=None):
        """(Ks, c2ws, nears, fars, ids, img_downscale) of the images `indices` (default: all): with their decoded photos in front, the
        arguments of datasets.images.build_train_buffers -- build_train_buffers(photos, *scene.train_buffer_args(indices))."""
        idx = np.arange(len(self.Ks)) if indices is None else np.asarray(indices, dtype=np.int64).reshape(-1)
        return ([self.Ks[i] for i in idx], [self.poses[i].astype(np.float32) for i in idx], [float(self.nears[i]) for i in idx],
                [float(self.fars[i]) for i in idx], [int(self.img_ids[i]) for i in idx], self.img_downscale)

    def eval_sample_args(self, index):
        """(K, c2w, near, far, image_id, img_downscale) of image `index`: with its decoded photo in front, the arguments of
        datasets.images.make_eval_sample; c2w is the float32 tensor the reference's sample carries (torch.FloatTensor(pose))."""
        i = int(index)
        return (self.Ks[i], torch.from_numpy(self.poses[i].astype(np.float32)), float(self.nears[i]), float(self.fars[i]),
                int(self.img_ids[i]), self.img_downscale)


def prepare_scene(qvecs, tvecs, cam_params, xyz_world, img_downscale, img_ids=None):
    """read_meta (:85-147) for the images given, in the order given, from their parsed COLMAP arrays: qvecs [N, 4] and tvecs [N, 3] of
    images.bin, cam_params [N, 4] = the PINHOLE (fx, fy, cx, cy) of each image's camera, xyz_world [P, 3] of points3D.bin (float64).
    Returns a Scene.  The scale is float32(max far) / 5 in float32; pose translations, nears, fars and xyz_world are divided by it in
    float64.  Raises ValueError naming the images that have no point in front of them (numpy warns there and yields NaN, which then
    poisons the scale of every image)."""
    w2c = world_to_camera(qvecs, tvecs)
    n = len(w2c)
    Ks = scaled_intrinsics(cam_params, img_downscale)
    if len(Ks) != n:
        raise ValueError("crnerf_amd.datasets.scene: %d poses but %d cameras" % (n, len(Ks)))
    ids = np.arange(n, dtype=np.int64) if img_ids is None else np.asarray(img_ids, dtype=np.int64).reshape(-1)
    if len(ids) != n:
        raise ValueError("crnerf_amd.datasets.scene: %d poses but %d image ids" % (n, len(ids)))
    if torch.is_tensor(xyz_world):
        xyz_host = xyz_world.detach().cpu().numpy()
    else:
        xyz_host = xyz_world = np.asarray(xyz_world)
    poses = camera_poses(w2c)
    nears, fars, counts = (t.cpu().numpy() for t in depth_bounds(xyz_world, w2c))
    empty = np.flatnonzero(counts == 0)
    if len(empty):
        raise ValueError("crnerf_amd.datasets.scene: no point of the sparse model lies in front of image(s) %s (of %d): near and far are "
                         "undefined there; drop those images or check their poses" % (empty.tolist(), n))
    max_far = fars.astype(np.float32).max()
    scale_factor = np.float32(max_far / np.float32(5))
    s = np.float64(scale_factor)
    poses[..., 3] /= s
    return Scene(Ks=Ks, poses=poses, nears=nears / s, fars=fars / s, xyz_world=xyz_host.astype(np.float64) / s, scale_factor=scale_factor,
                 img_ids=ids, img_downscale=int(img_downscale))

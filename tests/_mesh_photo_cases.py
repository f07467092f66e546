"""What the photo-colour tests share (csrc/crnerf_mesh_photo.h): the header's rules restated in NumPy float64 / int64, operation by operation --
written from the header, not from the kernels --, cameras, and hand cases small enough to follow with a pencil.

    project_ref(x, cam, z_near)                                       (d [n,3], u, v, z, front) of points x [n,3] float32 in one view
    zbuffer_ref(v, f, cams, dims, offsets, total, z_near)             the flat float32 depth buffer
    colors_ref(v, normals, photos, depth, cams, dims, offsets, total, z_near, depth_tol)      (colors [V,3] float32, views [V] int32)

NumPy rounds every float64 operation on its own, rint is ties-to-even, and a comparison with a NaN is false: the header's arithmetic."""
import numpy as np

MAX_SIDE = 16384
MAX_UV = 2.0 ** 20
INF = np.float32(np.inf)


# ---------------------------------------------------------------------------------------------------------------- cameras
def cam_row(fx, fy, cx, cy, c2w):
    """The 16 doubles of a view: fx, fy, cx, cy, R = c2w[:, :3] row-major, t = c2w[:, 3]."""
    c2w = np.asarray(c2w, np.float64).reshape(3, 4)
    return np.concatenate(([fx, fy, cx, cy], c2w[:, :3].reshape(9), c2w[:, 3])).astype(np.float64)


def look_at(eye, target, up=(0.0, 0.0, 1.0)):
    """c2w [3,4] of a camera at `eye` looking at `target`: columns right, up, back (the camera looks along -z), then the position."""
    eye, target, up = (np.asarray(a, np.float64) for a in (eye, target, up))
    back = eye - target
    back /= np.linalg.norm(back)
    right = np.cross(up, back)
    right /= np.linalg.norm(right)
    return np.stack((right, np.cross(back, right), back, eye), axis=1)


IDENTITY = np.concatenate((np.eye(3), np.zeros((3, 1))), axis=1)      # at the origin, looking along -z, x right, y up


def tables(views):
    """(cams [N,16] float64, dims [N,2] int32, offsets [N] int64, total) of [(cam_row, W, H)], the views one behind the other."""
    cams = np.stack([c for c, _, _ in views]).astype(np.float64) if views else np.zeros((0, 16))
    dims = np.array([[w, h] for _, w, h in views], np.int32).reshape(-1, 2)
    sizes = dims[:, 0].astype(np.int64) * dims[:, 1]
    offsets = np.concatenate(([0], np.cumsum(sizes)[:-1])).astype(np.int64) if views else np.zeros(0, np.int64)
    return cams, dims, offsets, int(sizes.sum())


def view_ok(W, H, off, total):
    return 2 <= W <= MAX_SIDE and 2 <= H <= MAX_SIDE and off >= 0 and off + W * H <= total


# ---------------------------------------------------------------------------------------------------------------- the rules
def project_ref(x, cam, z_near):
    x = np.asarray(x, np.float32).reshape(-1, 3)
    cam = np.asarray(cam, np.float64)
    fx, fy, cx, cy = cam[:4]
    R, t = cam[4:13].reshape(3, 3), cam[13:16]
    with np.errstate(all="ignore"):
        d = x.astype(np.float64) - t[None, :]
        c = [(d[:, 0] * R[0, k] + d[:, 1] * R[1, k]) + d[:, 2] * R[2, k] for k in range(3)]
        z = -c[2]
        u = cx + fx * (c[0] / z)
        v = cy - fy * (c[1] / z)
        front = z >= z_near
    return d, u, v, z, front


def valid_faces(f, V):
    f = np.asarray(f, np.int64).reshape(-1, 3)
    return f[((f >= 0) & (f < V)).all(axis=1)]


def _orient(Xa, Ya, Xb, Yb, Xc, Yc):
    return (Xb - Xa) * (Yc - Ya) - (Yb - Ya) * (Xc - Xa)


def zbuffer_ref(v, f, cams, dims, offsets, total, z_near):
    v = np.asarray(v, np.float32).reshape(-1, 3)
    faces = valid_faces(f, len(v))
    depth = np.full(total, INF, np.float32)
    for n in range(len(cams)):
        W, H, off = int(dims[n][0]), int(dims[n][1]), int(offsets[n])
        if not view_ok(W, H, off, total):
            continue
        view = depth[off:off + W * H].reshape(H, W)
        _, u, vv, z, front = project_ref(v, cams[n], z_near)
        with np.errstate(all="ignore"):
            ok = front & (np.abs(u) < MAX_UV) & (np.abs(vv) < MAX_UV)
        for a, b, c in faces[ok[faces].all(axis=1)]:
            ids = [a, b, c]
            X = [int(np.rint(u[k] * 16.0)) for k in ids]
            Y = [int(np.rint(vv[k] * 16.0)) for k in ids]
            zz = [z[k] for k in ids]
            A = _orient(X[0], Y[0], X[1], Y[1], X[2], Y[2])
            if A == 0:
                continue
            if A < 0:
                X[1], X[2], Y[1], Y[2], zz[1], zz[2], A = X[2], X[1], Y[2], Y[1], zz[2], zz[1], -A
            i0, i1 = max(0, -(-min(X) // 16)), min(W - 1, max(X) // 16)
            j0, j1 = max(0, -(-min(Y) // 16)), min(H - 1, max(Y) // 16)
            if i0 > i1 or j0 > j1:
                continue
            Px = (16 * np.arange(i0, i1 + 1, dtype=np.int64))[None, :]
            Py = (16 * np.arange(j0, j1 + 1, dtype=np.int64))[:, None]
            E0 = _orient(X[1], Y[1], X[2], Y[2], Px, Py)
            E1 = _orient(X[2], Y[2], X[0], Y[0], Px, Py)
            E2 = _orient(X[0], Y[0], X[1], Y[1], Px, Py)
            assert ((E0 + E1 + E2) == A).all()
            covered = (E0 >= 0) & (E1 >= 0) & (E2 >= 0)
            if not covered.any():
                continue
            with np.errstate(all="ignore"):
                w0, w1, w2 = (E.astype(np.float64) / np.float64(A) for E in (E0, E1, E2))
                iz = (w0 / zz[0] + w1 / zz[1]) + w2 / zz[2]
                D = (1.0 / iz).astype(np.float32)
            box = view[j0:j1 + 1, i0:i1 + 1]
            box[covered] = np.minimum(box[covered], D[covered])
    return depth


def colors_ref(v, normals, photos, depth, cams, dims, offsets, total, z_near, depth_tol):
    v = np.asarray(v, np.float32).reshape(-1, 3)
    V = len(v)
    S = np.zeros((V, 3), np.int64)
    cnt = np.zeros(V, np.int64)
    s = 1.0 + np.float64(depth_tol)
    facing = None
    if normals is not None:
        nrm = np.asarray(normals, np.float32).reshape(-1, 3).astype(np.float64)
        with np.errstate(all="ignore"):
            facing = ~((nrm == 0.0).all(axis=1))
    for n in range(len(cams)):
        W, H, off = int(dims[n][0]), int(dims[n][1]), int(offsets[n])
        if not view_ok(W, H, off, total):
            continue
        d, u, vv, z, front = project_ref(v, cams[n], z_near)
        with np.errstate(all="ignore"):
            ok = front.copy()
            if facing is not None:
                g = -((nrm[:, 0] * d[:, 0] + nrm[:, 1] * d[:, 1]) + nrm[:, 2] * d[:, 2])
                ok &= ~facing | (g > 0.0)
            ok &= (u >= 0.0) & (u <= W - 1) & (vv >= 0.0) & (vv <= H - 1)
        idx = np.nonzero(ok)[0]
        uu, vk, zk = u[idx], vv[idx], z[idx]
        if depth is not None:
            D = np.asarray(depth, np.float32)[off:off + W * H].reshape(H, W)[np.rint(vk).astype(np.int64), np.rint(uu).astype(np.int64)]
            with np.errstate(all="ignore"):
                keep = zk <= D.astype(np.float64) * s
            idx, uu, vk = idx[keep], uu[keep], vk[keep]
        x0 = np.minimum(np.floor(uu).astype(np.int64), W - 2)
        y0 = np.minimum(np.floor(vk).astype(np.int64), H - 2)
        a, b = uu - x0, vk - y0
        img = np.asarray(photos, np.uint8).reshape(-1, 3)[off:off + W * H].reshape(H, W, 3).astype(np.float64)
        for c in range(3):
            p00, p10, p01, p11 = img[y0, x0, c], img[y0, x0 + 1, c], img[y0 + 1, x0, c], img[y0 + 1, x0 + 1, c]
            top = p00 + a * (p10 - p00)
            bot = p01 + a * (p11 - p01)
            val = top + b * (bot - top)
            S[idx, c] += np.rint(val * 65536.0).astype(np.int64)
        cnt[idx] += 1
    colors = np.zeros((V, 3), np.float32)
    seen = cnt > 0
    colors[seen] = (S[seen].astype(np.float64) / (cnt[seen].astype(np.float64) * 16711680.0)[:, None]).astype(np.float32)
    return colors, cnt.astype(np.int32)


# ---------------------------------------------------------------------------------------------------------------- hand cases
# One camera for all of them: at the origin, looking along -z, fx = fy = 16, cx = cy = 0.  at(u, v, d) is the point that projects to pixel (u, v)
# at depth d: with d a power of two and u, v multiples of 1/16 every step of the projection is exact.
HAND_CAM = cam_row(16.0, 16.0, 0.0, 0.0, IDENTITY)


def at(u, v, d):
    return [u * d / 16.0, -v * d / 16.0, -d]


def _hand8_depth(t2=True):
    """8 x 8: the big triangle (0,0) (8,0) (0,8) at depth 2 covers i + j <= 8, its hypotenuse and corners included; the small one (2,2) (6,2) (2,6)
    at depth 1 covers i, j >= 2 with i + j <= 8."""
    j, i = np.mgrid[0:8, 0:8]
    want = np.where(i + j <= 8, np.float32(2.0), INF).astype(np.float32)
    if t2:
        want[(i >= 2) & (j >= 2) & (i + j <= 8)] = 1.0
    return want


def _hand8():
    v = [at(0, 0, 2), at(8, 0, 2), at(0, 8, 2),                  # 0-2: the big triangle, counter-clockwise on the screen (v runs down)
         at(2, 2, 1), at(6, 2, 1), at(2, 6, 1),                  # 3-5: the small one, nearer
         at(1, 1, 0.5), at(3, 3, 0.5), at(5, 5, 0.5),            # 6-8: collinear, nearer still: A = 0
         [-0.4375, 0.0, 1.0],                                    # 9: behind the camera; without the in-front test it would land on pixel (7, 0)
         at(2.0 ** 21, 1, 0.5)]                                  # 10: beyond 2^20 pixels
    f = [[0, 1, 2], [3, 5, 4],                                   # either winding
         [6, 7, 8],                                              # degenerate
         [0, 1, 11], [-1, 1, 2],                                 # an id outside [0, V)
         [6, 7, 9],                                              # one corner behind the camera: dropped, not clipped -- drawn from (1,1) (3,3) (7,0)
                                                                 # it would put depths below 1 on (1,1), (2,2), (3,3) and their neighbours
         [6, 10, 5]]                                             # one corner beyond 2^20 pixels: dropped
    return dict(v=v, f=f, views=[(HAND_CAM, 8, 8)], depth=_hand8_depth().reshape(-1))


def _tiny():
    """The smallest view, 2 x 2: corners on three of its four pixels; (1,1) is outside."""
    return dict(v=[at(0, 0, 4), at(1, 0, 4), at(0, 1, 4)], f=[[0, 1, 2]], views=[(HAND_CAM, 2, 2)], depth=np.array([4, 4, 4, np.inf], np.float32))


def _edge():
    """A pixel exactly on an edge and on a corner, off the lattice of whole pixels: corners (0.5, 0.5) (4.5, 0.5) (0.5, 4.5) hold no pixel
    centre on their legs; the hypotenuse i + j = 5 runs through (1,4) (2,3) (3,2) (4,1).  And a sliver (5,5) (7,5) (7,5.0625) that touches
    pixels (5,5), (6,5) and (7,5) along its lower edge only."""
    j, i = np.mgrid[0:8, 0:8]
    want = np.where((i >= 1) & (j >= 1) & (i + j <= 5), np.float32(2.0), INF).astype(np.float32)
    want[5, 5:8] = 8.0
    v = [at(0.5, 0.5, 2), at(4.5, 0.5, 2), at(0.5, 4.5, 2), at(5, 5, 8), at(7, 5, 8), at(7, 5.0625, 8)]
    return dict(v=v, f=[[0, 1, 2], [3, 4, 5]], views=[(HAND_CAM, 8, 8)], depth=want.reshape(-1))


def _skipped():
    """Two good views (8 x 8 at 0, 2 x 2 at 64) with a skipped view of each kind between them: W = 1, a negative offset, an offset past the buffer."""
    v = [at(0, 0, 2), at(8, 0, 2), at(0, 8, 2)]
    cams = np.stack([HAND_CAM] * 5)
    dims = np.array([[8, 8], [1, 8], [8, 8], [8, 8], [2, 2]], np.int32)
    offsets = np.array([0, 0, -5, 68 - 63, 64], np.int64)
    want = np.concatenate((_hand8_depth(False).reshape(-1), np.full(4, 2.0, np.float32)))
    return dict(v=v, f=[[0, 1, 2]], tables=(cams, dims, offsets, 68), depth=want)


HAND = {"two triangles and the dropped faces": _hand8, "the smallest view": _tiny, "edges and corners": _edge, "skipped views": _skipped}


def hand(name):
    case = HAND[name]()
    case["v"] = np.asarray(case["v"], np.float32)
    case["f"] = np.asarray(case["f"], np.int32)
    if "tables" not in case:
        case["tables"] = tables(case.pop("views"))
    case["z_near"] = 2.0 ** -4
    return case


def ramp(W, H):
    """The photo whose three channels are i + j (W + H <= 256): bilinear interpolation of it is u + v wherever the sample lies."""
    assert W + H <= 256
    j, i = np.mgrid[0:H, 0:W]
    return np.repeat((i + j).astype(np.uint8)[:, :, None], 3, axis=2)


RAMP_TOL = 2.0 ** -17 / 255 + 2.0 ** -24      # the rounding of q to 1/65536 of a grey level, and one float32 rounding below 1


# ---------------------------------------------------------------------------------------------------------------- scenes for the GPU tests
def sphere_views(inside):
    """Three views of different sizes (64 x 48, 33 x 40, 2 x 2) of the sphere of tests/_mesh_cases.py (radius 0.7 about the origin): from outside
    looking in, or from inside looking out."""
    if inside:
        poses = [look_at((0.05, 0.0, 0.1), (1, 0.2, 0.1)), look_at((-0.1, 0.1, 0.0), (0, -1, 0.3)), look_at((0, 0, 0), (0.3, 0.2, -1), up=(0, 1, 0))]
        focal = (30.0, 24.0, 1.5)
    else:
        poses = [look_at((2.5, 0.0, 0.0), (0, 0, 0)), look_at((-1.2, 1.7, 0.9), (0.1, 0, 0)), look_at((0.2, -0.3, 2.2), (0, 0, 0), up=(0, 1, 0))]
        focal = (60.0, 45.0, 2.0)
    sizes = ((64, 48), (33, 40), (2, 2))
    return [(cam_row(fo, fo * 1.03125, (w - 1) / 2 + 0.25, (h - 1) / 2 - 0.125, p), w, h) for fo, p, (w, h) in zip(focal, poses, sizes)]


def noise_photos(views, seed):
    """A flat [total,3] uint8 buffer of seeded noise for [(cam, W, H)]."""
    total = sum(w * h for _, w, h in views)
    return np.random.default_rng(seed).integers(0, 256, (total, 3), dtype=np.uint8)


def sub_pixel_mesh(W, H, n=4096, seed=11):
    """One triangle that covers all of a W x H view of HAND_CAM at depth 4, and n small faces (a fraction of a pixel to two pixels across) scattered in front
    of it at depths 1 to 3: (vertices, faces)."""
    rng = np.random.default_rng(seed)
    v = [at(-8, -8, 4), at(2 * W + 16, -8, 4), at(-8, 2 * H + 16, 4)]
    f = [[0, 1, 2]]
    for k in range(n):
        c = rng.uniform((0, 0), (W - 1, H - 1))
        depth = rng.uniform(1.0, 3.0)
        size = rng.choice([0.2, 0.6, 1.1, 2.3])
        for _ in range(3):
            p = c + rng.uniform(-size, size, 2)
            v.append(at(p[0], p[1], depth * rng.uniform(0.98, 1.02)))
        f.append([3 + 3 * k, 4 + 3 * k, 5 + 3 * k] if k % 2 else [3 + 3 * k, 5 + 3 * k, 4 + 3 * k])
    return np.asarray(v, np.float32), np.asarray(f, np.int32)

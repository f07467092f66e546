"""GPU checks of mesh smoothing and face normals (csrc/crnerf_mesh_smooth.h, ops.mesh_smooth, ops.mesh_vertex_normals,
crnerf_amd.geometry Mesh.smooth / recompute_normals, extract_mesh(smooth_steps=)).  Positions are compared bit for bit with the NumPy restatement
(tests/_mesh_smooth_cases.py); normals to within 2^-23 absolute per component -- one float32 ulp at 1, the bar of the simplified normals, whose
finish is the same: the only inexact steps are a float64 sqrt, a float64 division and the final rounding.

  1. Hand cases.   2. Extracted meshes: sphere(17) and plane(17) at 1, 2 and 10 steps, blobs(33).   3. One hot vertex: 20,000 faces around it.
  4. Past the chunk of the block-total scan: 1,164,962 vertices, 2,391,620 faces.   5. Determinism and the order of the faces.
  6. Guards behind the workspace and the outputs.   7. The Python layer: Mesh.smooth, recompute_normals, colorize, parts / PLY, extract_mesh.
"""
import ctypes

import numpy as np
import pytest
import torch

from crnerf_amd import _lib, geometry, ops
import crnerf_amd.synth as synth
from crnerf_amd.models.linearStyleTransfer import style_net
from crnerf_amd.models.nerf import NeRF_sigma

import _geometry_cases as G
import _mesh_cases as M
import _mesh_parts_cases as C
import _mesh_smooth_cases as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NORMAL_TOL = 2.0 ** -23
DEFAULTS = (0.5, -0.53)


def dev(a):
    return torch.from_numpy(np.array(a, copy=True, order="C")).to(DEV)      # (a copy: the shared references are read-only)


def same(got, want, what):
    """Equal shape, dtype and bytes; got: a device tensor."""
    g = got.cpu().numpy()
    assert g.dtype == want.dtype and g.shape == want.shape, (what, g.dtype, want.dtype, g.shape, want.shape)
    if g.tobytes() != np.ascontiguousarray(want).tobytes():
        bad = np.nonzero((g != want).any(axis=1))[0]
        raise AssertionError("%s: %d of %d rows differ, the first at %d: %r, want %r" % (what, len(bad), len(g), bad[0], g[bad[0]], want[bad[0]]))


def close_normals(got, want, what):
    g = got.cpu().numpy()
    assert g.dtype == np.float32 and g.shape == want.shape, (what, g.dtype, g.shape, want.shape)
    worst = float(np.abs(g.astype(np.float64) - want.astype(np.float64)).max()) if g.size else 0.0
    print("%s: normals differ by at most %.3g (bound %.3g)" % (what, worst, NORMAL_TOL))
    assert worst <= NORMAL_TOL, (what, worst)


_EXTRACTED = {}


def extracted(name):
    """(vertices, faces) of a field of tests/_mesh_cases.py by the restatement of crnerf_mesh.h; computed once."""
    if name not in _EXTRACTED:
        v, f, _ = M.mesh_ref(*{"sphere17": lambda: M.sphere(17), "plane17": lambda: M.plane(17)}[name](), 0.0, want_normals=False)
        _EXTRACTED[name] = (v, f)
    return _EXTRACTED[name]


# ---------------------------------------------------------------- 1. hand cases
@pytest.mark.parametrize("name", sorted(S.HAND))
def test_hand_cases(name):
    case = S.hand(name)
    v, f = case["v"], case["f"]
    args = (case["lo"], case["k"], case["steps"], case["lam"], case["mu"])
    want = S.smooth_ref(v, f, *args, case["pin"])
    assert np.array_equal(want, case["out"])
    d_v, d_f = dev(v), dev(f)
    got = ops.mesh_smooth(d_v, d_f, *args, pin_border=case["pin"])
    assert got.dtype == torch.float32 and got.shape == d_v.shape and got.is_contiguous() and got.device == torch.device(DEV)
    same(got, want, name)
    same(got, case["out"], (name, "by hand"))
    same(d_v, v, (name, "the input is untouched"))
    for pin in (True, False):                                  # the other setting of pin_border, and a full Taubin step or two
        for steps in (1, 2):
            same(ops.mesh_smooth(d_v, d_f, case["lo"], case["k"], steps, *DEFAULTS, pin_border=pin),
                 S.smooth_ref(v, f, case["lo"], case["k"], steps, *DEFAULTS, pin), (name, pin, steps))
    close_normals(ops.mesh_vertex_normals(d_v, d_f, 10), S.normals_ref(v, f, 10), name)


def test_the_triangle_moves_only_without_pin_border_and_zero_steps_is_the_round_trip():
    v, f = dev(S.hand("one triangle free")["v"]), dev(S.hand("one triangle free")["f"])
    assert torch.equal(ops.mesh_smooth(v, f, (0, 0, 0), 4, 3, *DEFAULTS, pin_border=True), v)
    assert not torch.equal(ops.mesh_smooth(v, f, (0, 0, 0), 4, 3, *DEFAULTS, pin_border=False), v)
    case = S.hand("steps = 0")
    got = ops.mesh_smooth(dev(case["v"]), dev(case["f"]), case["lo"], case["k"], 0, 0.5, 0.0)
    assert got.tolist() == [[0.3125, 1.0, 2.6875], [4.0, 0.0, 0.0], [0.0, 4.0, 0.0]] and not np.array_equal(got.cpu().numpy(), case["v"])
    # at the lattice Mesh.smooth picks, the round trip moves a coordinate of this size by about 1e-9: not a byte copy, and far below a float32 ulp
    lo, k, _ = S.box_of(case["v"])
    trip = ops.mesh_smooth(dev(case["v"]), dev(case["f"]), lo, k, 0, 0.5, 0.0).cpu().numpy()
    assert np.array_equal(trip, S.smooth_ref(case["v"], case["f"], lo, k, 0, 0.5, 0.0)) and np.abs(trip.astype(np.float64) - case["v"]).max() < 2.0 ** -24
    # Mesh.smooth(0) does not make that trip: it hands the mesh back
    mesh = geometry.Mesh(dev(case["v"]), dev(case["f"]))
    assert mesh.smooth(0) is mesh


def test_an_empty_mesh_and_a_mesh_without_faces():
    e3, f0 = torch.zeros(0, 3, device=DEV), torch.zeros(0, 3, dtype=torch.int32, device=DEV)
    assert ops.mesh_smooth(e3, f0, (0, 0, 0), 4, 2, *DEFAULTS).shape == (0, 3) and ops.mesh_vertex_normals(e3, dev(np.asarray(S.TET_F, np.int32)), 4).shape == (0, 3)
    got = geometry.Mesh(e3, f0, e3).smooth(2)
    assert got.vertices.shape == (0, 3) and got.normals.shape == (0, 3) and got.faces is f0
    case = S.hand("no faces")
    dust = geometry.Mesh(dev(case["v"]), f0, dev(case["v"]), dev(case["v"]))
    got = dust.smooth(2)
    lo, k, _ = S.box_of(case["v"])
    same(got.vertices, S.smooth_ref(case["v"], case["f"], lo, k, 0, 0.5, 0.0), "dust")      # nothing has a neighbour: the round trip
    assert not got.normals.any() and got.colors is dust.colors


# ---------------------------------------------------------------- 2. extracted meshes
@pytest.mark.parametrize("steps", [1, 2, 10])
@pytest.mark.parametrize("name", ["sphere17", "plane17"])
def test_extracted_meshes(name, steps):
    v, f = extracted(name)
    lo, k, k2 = S.box_of(v)
    pinned = S.pinned_ref(f, len(v))
    assert len(v) == {"sphere17": 1730, "plane17": 1089}[name] and pinned.sum() == {"sphere17": 0, "plane17": 128}[name]
    d_v, d_f = dev(v), dev(f)
    want = S.smooth_ref(v, f, lo, k, steps, *DEFAULTS)
    got = ops.mesh_smooth(d_v, d_f, lo, k, steps, *DEFAULTS)
    same(got, want, (name, steps))
    trip = S.smooth_ref(v, f, lo, k, 0, *DEFAULTS)
    assert np.array_equal(want[pinned], trip[pinned]) and (want[~pinned] != trip[~pinned]).any(axis=1).mean() > 0.9      # the border stays, the rest moves
    if name == "plane17":
        free = S.smooth_ref(v, f, lo, k, steps, *DEFAULTS, False)
        assert not np.array_equal(free[pinned], trip[pinned])
        same(ops.mesh_smooth(d_v, d_f, lo, k, steps, *DEFAULTS, pin_border=False), free, (name, steps, "free"))
    close_normals(ops.mesh_vertex_normals(got, d_f, k2), S.normals_ref(want, f, k2), (name, steps))
    mesh = geometry.Mesh(d_v, d_f).smooth(steps)                # the box Mesh.smooth picks is box_of's
    same(mesh.vertices, want, (name, steps, "Mesh.smooth"))
    assert mesh.normals is None and mesh.faces is d_f


def test_the_smoothed_sphere_keeps_its_shape_and_its_normals_point_outward():
    v, f = extracted("sphere17")
    mesh = geometry.Mesh(dev(v), dev(f)).recompute_normals().smooth(10)
    out, n = mesh.vertices.cpu().numpy().astype(np.float64), mesh.normals.cpu().numpy().astype(np.float64)
    r = np.linalg.norm(out, axis=1)
    ratio = S.volume(out, f) / S.volume(v, f)
    off = float(np.abs(n - out / r[:, None]).max())
    print("sphere(17) after 10 steps on the device: radii [%.5f, %.5f], volume x %.5f, normals within %.4f of radial" % (r.min(), r.max(), ratio, off))
    # the restatement's own figures at this size, measured on the CPU: [0.69293, 0.70235], 1.00487, 0.0702; the device equals it bit for bit above
    assert 0.692 < r.min() and r.max() < 0.703 and 1.004 < ratio < 1.006 and off < 0.071 and (np.einsum("ij,ij->i", n, out) > 0).all()


def test_blobs_six_parts_one_open():
    v, f, _ = C.mesh("blobs33")
    parts = C.parts("blobs33")
    pinned = S.pinned_ref(f, len(v))
    once = np.unique(M.topology(f, len(v))["once"])
    assert len(parts[2]) == 6 and 0 < len(once) < len(v) // 4 and np.array_equal(np.nonzero(pinned)[0], once)      # the border of the sphere the box cuts
    assert len(np.unique(parts[0][once])) == 1
    lo, k, k2 = S.box_of(v)
    want = S.smooth_ref(v, f, lo, k, 3, *DEFAULTS)
    mesh = geometry.Mesh(dev(v), dev(f), dev(np.zeros_like(v))).smooth(3)
    same(mesh.vertices, want, "blobs33")
    close_normals(mesh.normals, S.normals_ref(want, f, k2), "blobs33")


# ---------------------------------------------------------------- 3. one hot vertex
def test_one_hot_vertex_the_long_row_and_every_degree_add_on_one_address():
    v, f = S.fan(20000)
    d, h = S.adjacency_ref(f, len(v))
    assert d[0] == 40000 and d[1:].tolist() == [4] * 20000 and h[0] == 0 and (h[1:] != 0).all()
    lo, k, k2 = S.box_of(v)
    d_v, d_f = dev(v), dev(f)
    for pin, steps in ((True, 2), (False, 2), (False, 5)):
        want = S.smooth_ref(v, f, lo, k, steps, *DEFAULTS, pin)
        assert not np.array_equal(want[0], v[0])
        same(ops.mesh_smooth(d_v, d_f, lo, k, steps, *DEFAULTS, pin_border=pin), want, ("fan", pin, steps))
    close_normals(ops.mesh_vertex_normals(d_v, d_f, k2), S.normals_ref(v, f, k2), "fan")
    # the same fan with its faces shuffled: the hub's adds no longer come from neighbouring lanes
    perm = np.random.default_rng(4).permutation(len(f))
    same(ops.mesh_smooth(d_v, dev(f[perm]), lo, k, 2, *DEFAULTS, pin_border=False), S.smooth_ref(v, f, lo, k, 2, *DEFAULTS, False), "fan shuffled")
    # a row of exactly 64 entries, one of 66, and their neighbours: the switch between the two paths
    for n in (31, 32, 33, 40):
        v, f = S.fan(n)
        lo, k, _ = S.box_of(v)
        same(ops.mesh_smooth(dev(v), dev(f), lo, k, 3, *DEFAULTS, pin_border=False), S.smooth_ref(v, f, lo, k, 3, *DEFAULTS, False), ("fan", n))


# ---------------------------------------------------------------- 4. past the scan's chunk
def test_past_the_chunk_of_the_block_total_scan():
    v, f, _ = C.mesh("noise73+0.35")
    assert (len(v), len(f)) == (1164962, 2391620) and len(v) > 1024 * 1024
    lo, k, k2 = S.box_of(v)
    want = S.smooth_ref(v, f, lo, k, 2, *DEFAULTS)
    mesh = geometry.Mesh(dev(v), dev(f)).recompute_normals().smooth(2)
    same(mesh.vertices, want, "noise73")
    close_normals(mesh.normals, S.normals_ref(want, f, k2), "noise73")


# ---------------------------------------------------------------- 5. determinism
def test_two_runs_give_equal_bytes_and_the_order_of_the_faces_does_not_matter():
    v, f, _ = C.mesh("noise41-0.6")
    lo, k, k2 = S.box_of(v)
    d_v = dev(v)
    mesh = geometry.Mesh(d_v, dev(f), d_v)
    a, b = mesh.smooth(4), mesh.smooth(4)
    for name in ("vertices", "normals"):
        assert getattr(a, name).cpu().numpy().tobytes() == getattr(b, name).cpu().numpy().tobytes(), name
    want = S.smooth_ref(v, f, lo, k, 4, *DEFAULTS)
    same(a.vertices, want, "noise41")
    perm = np.random.default_rng(3).permutation(len(f))
    shuffled = np.roll(f[perm], 1, axis=1)                      # another order, and another first corner
    c = geometry.Mesh(d_v, dev(shuffled), d_v).smooth(4)
    same(c.vertices, want, "faces shuffled")
    assert c.normals.cpu().numpy().tobytes() == a.normals.cpu().numpy().tobytes()      # bit for bit between the two device runs
    close_normals(a.normals, S.normals_ref(want, f, k2), "noise41")


# ---------------------------------------------------------------- 6. guards
def test_nothing_is_written_behind_the_workspace_or_the_outputs():
    v, f, _ = C.mesh("blobs33")
    V, F = len(v), len(f)
    lo, k, k2 = S.box_of(v)
    lo32 = [float(np.float32(x)) for x in lo]
    lib = _lib.load()
    p = lambda t: ctypes.c_void_p(t.data_ptr())      # noqa: E731
    nbytes = lib.crnerf_mesh_smooth_workspace_bytes(V, F)
    assert nbytes >= 80 * V + 24 * F and nbytes % 8 == 0
    ws = torch.full((nbytes + 64,), 0x5a, dtype=torch.uint8, device=DEV)          # a guard behind the workspace
    d_v, d_f = dev(v), dev(f)
    out = torch.full((V + 1, 3), -7.0, device=DEV)                                # a guard row behind each output
    nrm = torch.full((V + 1, 3), -7.0, device=DEV)
    st = _lib.stream_ptr()
    _lib.check(lib.crnerf_mesh_adjacency_i32(p(d_f), V, F, p(ws), st), "adjacency")
    for steps, pin in ((0, 1), (1, 1), (3, 0)):                                   # one adjacency, several smooths
        _lib.check(lib.crnerf_mesh_smooth_f32(p(d_v), V, F, *lo32, k, steps, 0.5, -0.53, pin, p(ws), p(out), st), "smooth")
        same(out[:V], S.smooth_ref(v, f, lo, k, steps, *DEFAULTS, bool(pin)), ("C level", steps, pin))
        _lib.check(lib.crnerf_mesh_vertex_normals_f32(p(out), p(d_f), V, F, k2, p(ws), p(nrm), st), "normals")      # in between: it leaves the adjacency alone
    close_normals(nrm[:V], S.normals_ref(S.smooth_ref(v, f, lo, k, 3, *DEFAULTS, False), f, k2), "C level")
    assert bool((out[V] == -7.0).all()) and bool((nrm[V] == -7.0).all())
    assert bool((ws[nbytes:] == 0x5a).all())
    # in place: out_vertices may be the vertices
    inplace = d_v.clone()
    _lib.check(lib.crnerf_mesh_smooth_f32(p(inplace), V, F, *lo32, k, 2, 0.5, -0.53, 1, p(ws), p(inplace), st), "smooth in place")
    same(inplace, S.smooth_ref(v, f, lo, k, 2, *DEFAULTS), "in place")
    same(d_v, v, "the input")


# ---------------------------------------------------------------- 7. the Python layer
class _Args:
    nerf_out_dim, img_wh = 64, [8, 8]


def _model(seed):
    m = NeRF_sigma("coarse", _Args(), in_channels_xyz=93, in_channels_dir=27).to(G.DEV)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in G.STATES[seed].items()})
    return m.eval()


def test_mesh_smooth_keeps_faces_and_colours_and_replaces_normals():
    v, f, n = C.mesh("blobs33")
    col = np.random.default_rng(17).uniform(0, 1, v.shape).astype(np.float32)
    lo, k, k2 = S.box_of(v)
    mesh = geometry.Mesh(dev(v), dev(f), dev(n), dev(col))
    got = mesh.smooth(2)
    want = S.smooth_ref(v, f, lo, k, 2, *DEFAULTS)
    assert got is not mesh and got.faces is mesh.faces and got.colors is mesh.colors and got.normals is not mesh.normals
    same(got.vertices, want, "smooth")
    close_normals(got.normals, S.normals_ref(want, f, k2), "smooth")
    for t, w in ((mesh.vertices, v), (mesh.faces, f), (mesh.normals, n), (mesh.colors, col)):      # the original is untouched
        same(t, w, "original")
    bare = geometry.Mesh(mesh.vertices, mesh.faces).smooth(2, pin_border=False)
    assert bare.normals is None and bare.colors is None
    same(bare.vertices, S.smooth_ref(v, f, lo, k, 2, *DEFAULTS, False), "bare")
    same(mesh.smooth(1, lam=0.3, mu=-0.31).vertices, S.smooth_ref(v, f, lo, k, 1, 0.3, -0.31), "other weights")
    # face normals of an extracted mesh agree with its density-gradient normals in direction: both point out of the dense region
    again = mesh.recompute_normals()
    assert again.vertices is mesh.vertices and again.faces is mesh.faces and again.colors is mesh.colors
    close_normals(again.normals, S.normals_ref(v, f, k2), "recompute")
    assert float(((again.normals * mesh.normals).sum(dim=1) > 0.5).float().mean()) > 0.95


@torch.no_grad()
def test_recompute_normals_on_a_mesh_built_without_them_then_colorize():
    v, f = extracted("sphere17")
    mesh = geometry.Mesh(dev(v), dev(f))
    model = _model(21)
    decoder = style_net(_Args()).to(G.DEV)
    decoder.load_state_dict({k: torch.from_numpy(t) for k, t in synth.decoder_state(3).items()})
    decoder.eval()
    style = torch.from_numpy(np.random.default_rng(0).uniform(0, 1, (1, 64, 32, 32)).astype(np.float32)).to(G.DEV)
    with pytest.raises(ValueError, match="no normals"):
        mesh.colorize(model, decoder, style)
    ready = mesh.recompute_normals()
    close_normals(ready.normals, S.normals_ref(v, f, S.box_of(v)[2]), "sphere17")
    coloured = ready.colorize(model, decoder, style)
    assert coloured.colors.shape == (len(v), 3) and float(coloured.colors.min()) >= 0.0 and float(coloured.colors.max()) <= 1.0
    assert torch.equal(coloured.colors, geometry.point_colors(model, decoder, style, ready.vertices, -ready.normals))
    smoothed = coloured.smooth(2)
    assert smoothed.colors is coloured.colors and smoothed.normals is not None


def test_simplify_then_smooth_then_parts_and_a_ply(tmp_path):
    v, f, n = C.mesh("blobs33")
    mesh = geometry.Mesh(dev(v), dev(f), dev(n))
    small = mesh.largest(5).simplify(0.125, lo=(-1, -1, -1), hi=(1, 1, 1))
    sv, sf = small.vertices.cpu().numpy(), small.faces.cpu().numpy()
    lo, k, k2 = S.box_of(sv)
    smooth = small.smooth(3)
    want = S.smooth_ref(sv, sf, lo, k, 3, *DEFAULTS)
    same(smooth.vertices, want, "simplify then smooth")
    close_normals(smooth.normals, S.normals_ref(want, sf, k2), "simplify then smooth")
    moved = np.linalg.norm(want.astype(np.float64) - sv, axis=1)
    assert 0 < moved.max() < 0.125                             # the blocks go, nothing travels a cell
    parts = smooth.parts()
    ref = C.parts_ref(sf, len(sv))
    assert parts.count == len(ref[2]) and parts.n_faces.tolist() == ref[3].tolist()      # smoothing changes no connectivity
    path = str(tmp_path / "smooth.ply")
    smooth.save_ply(path)
    with open(path, "rb") as fh:
        blob = fh.read()
    end = blob.index(b"end_header\n") + 11
    V, F = len(sv), len(sf)
    assert b"element vertex %d\n" % V in blob[:end] and b"property float nz\n" in blob[:end] and end + 24 * V + 13 * F == len(blob)
    rows = np.frombuffer(blob, dtype="<f4", count=6 * V, offset=end).reshape(V, 6)
    assert np.array_equal(rows[:, :3], want) and np.array_equal(rows[:, 3:], smooth.normals.cpu().numpy())


def test_extract_mesh_smooth_steps():
    m = _model(22)
    lo, hi, res = (-1.0, -0.5, 0.25), (1.0, 1.5, 2.0), (11, 6, 9)
    thr = float(geometry.density_grid(m, lo, hi, res).sigma.median())
    today = geometry.density_grid(m, lo, hi, res).mesh(thr)
    names = ("vertices", "faces", "normals")
    for name in names:          # the default keeps today's result byte for byte
        assert torch.equal(getattr(geometry.extract_mesh(m, lo, hi, res, thr, smooth_steps=0), name), getattr(today, name)), name
    for kw, by_hand in ((dict(), today.smooth(2)), (dict(keep_largest=True), today.largest().smooth(2)),
                        (dict(simplify_cell=0.5), today.simplify(0.5).smooth(2)),
                        (dict(keep_largest=True, simplify_cell=0.45), today.largest().simplify(0.45).smooth(2))):
        got = geometry.extract_mesh(m, lo, hi, res, thr, smooth_steps=2, **kw)
        for name in names:
            assert torch.equal(getattr(got, name), getattr(by_hand, name)), (kw, name)
        assert got.colors is None and got.vertices.shape[0] > 0
    # against the restatement, from the device's own mesh
    v, f = today.vertices.cpu().numpy(), today.faces.cpu().numpy()
    box = S.box_of(v)
    want = S.smooth_ref(v, f, box[0], box[1], 2, *DEFAULTS)
    got = geometry.extract_mesh(m, lo, hi, res, thr, smooth_steps=2)
    same(got.vertices, want, "extract_mesh")
    close_normals(got.normals, S.normals_ref(want, f, box[2]), "extract_mesh")
